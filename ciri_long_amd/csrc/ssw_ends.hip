// ssw_ends.hip -- K1g: end-anchored affine-gap alignment of pairs (global, semiglobal, overlap; start-anchored: prefix, extend) in
// int32 cells (gfx950).
//
// The row-scan form of K1w (ssw_scan_wide.hip) without its packing: one wave takes one pair, its 64 lanes own kEnCpl consecutive
// reference columns each (a chunk of kEnChunk columns), the loop runs over the query rows, and a longer reference is walked chunk
// after chunk, a chunk handing the H and E of its last column on, one pair of values per row (two buffers, written by one chunk
// and read by the next).  Per row step and lane:
//     F[k] = max(Hprev[k] - go, Fprev[k] - ge)                        lane-private
//     T[k] = max(diag[k] + s, F[k])                                   H without E
//     V    = max over k of T[k] - go + (p + 1) ge                     p = 8 lane + k, the column inside the chunk
//     u    = exclusive prefix maximum of V over the lanes (wave_prefix_max + one DPP move), lane 0 seeded with E of column 0
//     E[k] = u - p ge,  H[k] = max(T[k], E[k]),  u = max(u, T[k] - go + (p + 1) ge)
// -- E[j] = max(E[j-1] - ge, H[j-1] - go) as a max-plus scan in the frame E[p] + p ge, exact because go >= ge lets T stand for H.
// No cell holds minus infinity: F of row 0 and E of column 0 enter as H - go, which gives the same first F and E, so every value
// is the score of an alignment (or one gap opening below it) and the host's bound (m + n) max(|s|, go, ge) < 2^30 keeps int32.
// The mode is a template parameter: the boundary values, and which end cells are followed (the last row's running maximum keyed
// by the smallest column, the last column's keyed by the smallest row in the lane that owns column n, the corner).
// prefix and extend have global's boundary.  prefix ends where semiglobal does, the last row's maximum seeded with H[m][0].  extend
// ends at the greatest H of all cells, smallest i, then smallest j, (0, 0) with 0 included: every lane keeps the best (value, i, k)
// of its own cells of a chunk under a bare > (rows ascend, columns ascend within a row: the first is the smallest key), joins it
// to the best it carries over the chunks by the key (a later chunk's columns are larger, its rows may be smaller), and the lanes
// are reduced once, after the last chunk.  Boundary cells but (0, 0) are <= 0 and lose every tie to (0, 0), the seed of every lane.
// STORE: each cell also leaves 4 bits -- H's source (0 diagonal, 1 E, 2 F; that order is the tie rule), "E opened here", "F opened
// here" -- one 32-bit word per lane and row, and ssw_ends_walk_kernel walks them back, one lane per pair (as K4t does): the walk
// itself is pr_walk in ssw_pairs.h, shared with K1gb, and the kernel here says where the word of a cell lies.
// tools/ends_model.py is this scheme in Python for any geometry; tests/ends_check.py is the definition.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "clh_device.h"
#include "clh_device_ops.h"
#include "ssw_pairs.h"

namespace clh {

static_assert(kEnCpl == 8, "a lane's row of decisions is one 32-bit word: 8 columns x 4 bits");

// H[0][j]: 0 on a free row, one gap of j letters in the global mode (unsigned arithmetic: lanes past column n hold garbage, not UB)
template <int MODE>
__device__ __forceinline__ int en_row0(int j, int go, int ge)
{
    return (en_anchored(MODE) && j > 0) ? (int)(0u - (uint32_t)go - (uint32_t)(j - 1) * (uint32_t)ge) : 0;
}
template <int MODE>
__device__ __forceinline__ int en_col0(int i, int go, int ge)
{
    return (MODE == EN_OVERLAP || i == 0) ? 0 : (int)(0u - (uint32_t)go - (uint32_t)(i - 1) * (uint32_t)ge);
}

template <int MODE, bool STORE>
__global__ void __launch_bounds__(64) ssw_ends_kernel(const EnParams prm, int first, int count)
{
    __shared__ int smat[32 * 32];                    // [query code][reference code]
    const int lane = threadIdx.x & 63;
    pr_load_matrix(smat, prm.mat, prm.n_mat, lane);
    const int x = (int)blockIdx.x;
    if (x >= count || first + x >= prm.npairs) return;
    const EnPair pr = prm.pairs[first + x];
    const int m = pr.m, n = pr.n;
    if (m <= 0 || n <= 0) return;                    // an empty side is answered by fetch
    const int go = prm.go, ge = prm.ge;
    const int nchunks = (n + kEnChunk - 1) / kEnChunk;
    const int mpad = (m + 63) & ~63;
    // hand-over buffers of this pair: [buffer 0 / 1][H / E][mpad]
    if (nchunks > 1 && (pr.hand_off < 0 || pr.hand_off + (int64_t)4 * mpad > prm.hand_cap)) return;
    int32_t* hand = prm.hand + (nchunks > 1 ? pr.hand_off : 0);
    const int8_t* qry = prm.qry + pr.q_off;
    const int8_t* ref = prm.ref + pr.r_off;
    bool ws_ok = true;
    if (STORE) {
        const int llast = (n - (nchunks - 1) * kEnChunk + kEnCpl - 1) / kEnCpl;
        const int64_t need = (int64_t)4 * m * ((int64_t)64 * (nchunks - 1) + llast);
        ws_ok = pr.ws_off >= 0 && (pr.ws_off & 3) == 0 && pr.ws_off + need <= prm.ws_cap;
    }

    int row_best = en_col0<MODE>(m, go, ge), row_j = 0;        // the last row's running maximum, smallest column
    int col_best = 0, col_i = 0, corner = 0;                   // the last column's (H[0][n] = 0 where it counts), smallest row; H[m][n]
    const int ln = ((n - 1) % kEnChunk) / kEnCpl, kn = ((n - 1) % kEnChunk) % kEnCpl;
    int ext_v = 0, ext_i = 0, ext_j = 0;                       // extend: the best cell this lane has seen, seeded with (0, 0)

    for (int c = 0; c < nchunks; ++c) {
        const int c0 = c * kEnChunk;
        const bool last = c == nchunks - 1;
        const int cols = last ? n - c0 : kEnChunk;
        const int L = (cols + kEnCpl - 1) / kEnCpl;            // lanes with a column
        int rcode[kEnCpl], off[kEnCpl], poff[kEnCpl], Hp[kEnCpl], Fp[kEnCpl];
#pragma unroll
        for (int k = 0; k < kEnCpl; ++k) {
            const int p = lane * kEnCpl + k, j = c0 + 1 + p;
            rcode[k] = j <= n ? ((int)ref[j - 1] & 31) : 0;
            poff[k] = (int)((uint32_t)p * (uint32_t)ge);
            off[k] = (int)((uint32_t)(p + 1) * (uint32_t)ge - (uint32_t)go);
            Hp[k] = en_row0<MODE>(j, go, ge);
            Fp[k] = Hp[k] - go;
        }
        int hleft = en_row0<MODE>(c0 + lane * kEnCpl, go, ge);           // H[i-1][first own column - 1]
        const int32_t* inH = hand + (size_t)((c + 1) & 1) * 2 * mpad;    // written by chunk c - 1
        const int32_t* inE = inH + mpad;
        int32_t* outHp = hand + (size_t)(c & 1) * 2 * mpad;
        int32_t* outEp = outHp + mpad;
        uint32_t* wsp = nullptr;
        if (STORE && ws_ok) wsp = (uint32_t*)(prm.ws + pr.ws_off) + (size_t)c * m * 64;
        const int own = cols - lane * kEnCpl;                  // extend: register k holds a column of the reference while k < own
        int cv = (int)0x80000000, ci = 0, ck = 0;              // extend: this chunk's best of the lane

        for (int i0 = 0; i0 < m; i0 += 64) {
            const bool mine = i0 + lane < m;
            const int qv = mine ? ((int)qry[i0 + lane] & 31) : 0;
            int vH = 0, vE = 0, outH = 0, outE = 0;
            if (c > 0 && mine) { vH = inH[i0 + lane]; vE = inE[i0 + lane]; }
            const int rows = m - i0 < 64 ? m - i0 : 64;
            for (int rr = 0; rr < rows; ++rr) {
                const int i = i0 + rr + 1;
                const int qc = __builtin_amdgcn_readlane(qv, rr);
                int hin, ein;                                            // H and E of the column in front of the chunk, this row
                if (c == 0) { hin = en_col0<MODE>(i, go, ge); ein = hin - go; }
                else { hin = __builtin_amdgcn_readlane(vH, rr); ein = __builtin_amdgcn_readlane(vE, rr); }
                const int E0 = pr_max(ein - ge, hin - go);
                const int* srow = smat + qc * 32;
                int T[kEnCpl], F[kEnCpl], D[kEnCpl], H[kEnCpl], E[kEnCpl];
                int v = 0;
#pragma unroll
                for (int k = 0; k < kEnCpl; ++k) {
                    F[k] = pr_max(Hp[k] - go, Fp[k] - ge);
                    D[k] = (k ? Hp[k - 1] : hleft) + srow[rcode[k]];
                    T[k] = pr_max(D[k], F[k]);
                    const int xk = T[k] + off[k];
                    v = k ? pr_max(v, xk) : xk;
                }
                v = lane == 0 ? pr_max(v, E0) : v;
                int u = dpp_shr1(E0, wave_prefix_max(v));                // lane 0 keeps E0
#pragma unroll
                for (int k = 0; k < kEnCpl; ++k) {
                    E[k] = u - poff[k];
                    H[k] = pr_max(T[k], E[k]);
                    u = pr_max(u, T[k] + off[k]);
                }
                const int nleft = dpp_shr1(hin, H[kEnCpl - 1]);          // H[i][first own column - 1]
                if (STORE) {
                    uint32_t w = 0;
#pragma unroll
                    for (int k = 0; k < kEnCpl; ++k) {
                        const int left = k ? H[k - 1] : nleft;
                        const uint32_t src = H[k] == D[k] ? 0u : (H[k] == E[k] ? 1u : 2u);
                        const uint32_t nib = src | (E[k] == left - go ? 4u : 0u) | (F[k] == Hp[k] - go ? 8u : 0u);
                        w |= nib << (4 * k);
                    }
                    if (wsp && lane < L) wsp[(size_t)(i - 1) * L + lane] = w;
                }
                if (!last) {
                    const int sH = __builtin_amdgcn_readlane(H[kEnCpl - 1], 63), sE = __builtin_amdgcn_readlane(E[kEnCpl - 1], 63);
                    outH = lane == rr ? sH : outH;                      // lane rr keeps row i0 + rr: one coalesced store per 64 rows
                    outE = lane == rr ? sE : outE;
                }
                if (MODE == EN_EXTEND) {
#pragma unroll
                    for (int k = 0; k < kEnCpl; ++k)
                        if (k < own && H[k] > cv) { cv = H[k]; ci = i; ck = k; }
                }
                if ((MODE == EN_SEMIGLOBAL || MODE == EN_OVERLAP || MODE == EN_PREFIX) && i == m) {
                    int bv = (int)0x80000000, bj = 0x7fffffff;
#pragma unroll
                    for (int k = 0; k < kEnCpl; ++k) {
                        const int j = c0 + 1 + lane * kEnCpl + k;
                        if (j <= n && H[k] > bv) { bv = H[k]; bj = j; }
                    }
#pragma unroll
                    for (int d = 1; d < 64; d <<= 1) {
                        const int v2 = __shfl_xor(bv, d), j2 = __shfl_xor(bj, d);
                        const bool take = v2 > bv || (v2 == bv && j2 < bj);
                        bv = take ? v2 : bv; bj = take ? j2 : bj;
                    }
                    if (bv > row_best) { row_best = bv; row_j = bj; }
                }
                if (last && (MODE == EN_OVERLAP || i == m)) {
                    int hn = H[0];
#pragma unroll
                    for (int k = 1; k < kEnCpl; ++k) hn = k == kn ? H[k] : hn;
                    if (i == m) corner = hn;
                    else if (hn > col_best) { col_best = hn; col_i = i; }    // meaningful in lane ln
                }
#pragma unroll
                for (int k = 0; k < kEnCpl; ++k) { Hp[k] = H[k]; Fp[k] = F[k]; }
                hleft = nleft;
            }
            if (!last && mine) { outHp[i0 + lane] = outH; outEp[i0 + lane] = outE; }
        }
        if (MODE == EN_EXTEND) {
            const bool take = cv > ext_v || (cv == ext_v && ci < ext_i);
            ext_v = take ? cv : ext_v; ext_i = take ? ci : ext_i; ext_j = take ? c0 + 1 + lane * kEnCpl + ck : ext_j;
        }
        if (!last) {      // the next chunk reads what other lanes of this wave stored
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            __syncthreads();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        }
    }
    corner = __shfl(corner, ln); col_best = __shfl(col_best, ln); col_i = __shfl(col_i, ln);
    int score, ei, ej;
    if (MODE == EN_GLOBAL) { score = corner; ei = m; ej = n; }
    else if (MODE == EN_EXTEND) {
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int v2 = __shfl_xor(ext_v, d), i2 = __shfl_xor(ext_i, d), j2 = __shfl_xor(ext_j, d);
            const bool take = v2 > ext_v || (v2 == ext_v && (i2 < ext_i || (i2 == ext_i && j2 < ext_j)));
            ext_v = take ? v2 : ext_v; ext_i = take ? i2 : ext_i; ext_j = take ? j2 : ext_j;
        }
        score = ext_v; ei = ext_i; ej = ext_j;
    }
    else if (MODE == EN_SEMIGLOBAL || MODE == EN_PREFIX || row_best >= col_best) { score = row_best; ei = m; ej = row_j; }     // last-row cells before last-column cells
    else { score = col_best; ei = col_i; ej = n; }
    if (lane == 0) {
        int32_t* row = prm.rows + (size_t)(first + x) * 8;
        row[0] = score;
        row[1] = en_anchored(MODE) ? 0 : -1;                      // begins: the walk's, unless the mode fixes them
        row[2] = ej - 1;
        row[3] = MODE == EN_OVERLAP ? -1 : 0;
        row[4] = ei - 1;
        row[5] = 0;
        row[6] = 0;
        row[7] = (STORE && !ws_ok) ? EN_ST_NO_WALK : 0;
    }
}

// one lane per pair: pr_walk over the words the storing form left, chunk after chunk, per chunk row after row, a word per lane
__global__ void ssw_ends_walk_kernel(const EnParams prm, int first, int count)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= count || first + x >= prm.npairs) return;
    const EnPair pr = prm.pairs[first + x];
    const int m = pr.m, n = pr.n;
    if (m <= 0 || n <= 0) return;
    int32_t* row = prm.rows + (size_t)(first + x) * 8;
    if (row[7] != 0) return;                                     // unwritten, or without stored decisions: fetch reports it
    const int nchunks = (n + kEnChunk - 1) / kEnChunk;
    const int llast = (n - (nchunks - 1) * kEnChunk + kEnCpl - 1) / kEnCpl;
    const int64_t nwords = (int64_t)m * ((int64_t)64 * (nchunks - 1) + llast);
    if (pr.ws_off < 0 || pr.ws_off + 4 * nwords > prm.ws_cap || pr.cig_off < 0 || pr.cig_off + pr.cig_cap > prm.cigar_cap) { row[7] = EN_ST_NO_WALK; return; }
    const uint32_t* ws = (const uint32_t*)(prm.ws + pr.ws_off);
    pr_walk(row, prm.mode, m, n, prm.cigar + pr.cig_off, pr.cig_cap, [&](int i, int j) -> int {
        const int ch = (j - 1) / kEnChunk, p = (j - 1) % kEnChunk;
        const int L = ch == nchunks - 1 ? llast : 64;
        const int64_t wi = (int64_t)ch * m * 64 + (int64_t)(i - 1) * L + p / kEnCpl;
        if (wi < 0 || wi >= nwords) return -1;
        return (int)((ws[wi] >> (4 * (p % kEnCpl))) & 15u);
    });
}

template <int MODE>
static void en_launch(const EnParams& p, bool store, int first, int count, hipStream_t st)
{
    if (store) hipLaunchKernelGGL((ssw_ends_kernel<MODE, true>), dim3(count), dim3(64), 0, st, p, first, count);
    else hipLaunchKernelGGL((ssw_ends_kernel<MODE, false>), dim3(count), dim3(64), 0, st, p, first, count);
}

hipError_t launch_ssw_ends(const EnParams& p, bool store, int first, int count, hipStream_t stream)
{
    if (count <= 0) return hipSuccess;
    if (p.mode == EN_GLOBAL) en_launch<EN_GLOBAL>(p, store, first, count, stream);
    else if (p.mode == EN_SEMIGLOBAL) en_launch<EN_SEMIGLOBAL>(p, store, first, count, stream);
    else if (p.mode == EN_OVERLAP) en_launch<EN_OVERLAP>(p, store, first, count, stream);
    else if (p.mode == EN_PREFIX) en_launch<EN_PREFIX>(p, store, first, count, stream);
    else if (p.mode == EN_EXTEND) en_launch<EN_EXTEND>(p, store, first, count, stream);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_ssw_ends_walk(const EnParams& p, int first, int count, hipStream_t stream)
{
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(ssw_ends_walk_kernel, dim3((count + 63) / 64), dim3(64), 0, stream, p, first, count);
    return hipGetLastError();
}

}  // namespace clh
