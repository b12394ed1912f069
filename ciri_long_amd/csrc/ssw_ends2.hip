// ssw_ends2.hip -- K1g under two-piece affine gap costs: a gap of k letters costs min(go1 + (k-1) ge1, go2 + (k-1) ge2) (gfx950).
//
// The sibling of ssw_ends_kernel (ssw_ends.hip), in a file of its own so that the one-piece instantiations compile as they did:
// the same geometry (one wave per pair, kEnCpl columns per lane, chunks of kEnChunk columns), the same modes, boundaries, end
// cells and tie rules.  What differs, per row step and lane:
//     F_p[k] = max(Hprev[k] - go_p, F_pprev[k] - ge_p)                p = 1, 2, lane-private
//     T[k]   = max(diag[k] + s, F_1[k], F_2[k])                       H without E
//     V_p    = max over k of T[k] - go_p + (c + 1) ge_p               c = 8 lane + k; two scans, each in its own frame E_p + c ge_p
//     u_p    = exclusive prefix maximum of V_p over the lanes, lane 0 seeded with E_p of the chunk's column 0; the two
//              wave_prefix_max chains are independent and the compiler interleaves them
//     e_p    = u_p - (8 lane) ge_p,  then along the lane  E_p[k] = e_p,  H[k] = max(T[k], E_1[k], E_2[k]),
//              e_p = max(e_p - ge_p, T[k] - go_p)
// The scan of piece p sees T - go_p and E_p - ge_p, not the definition's H - go_p: H may be the other piece's E.  Under the
// admitted costs 0 <= ge2 <= ge1 <= go1 <= go2 that cross term never reaches H and never changes a value the walk reads:
//     E_2[j'] - go1 - k ge1 <= E_2[j'] - (k + 1) ge2 <= E_2[j' + k + 1], and a piece-1 run of a + 1 letters followed by a piece-2 opening
//     costs go1 + a ge1 + go2 + k ge2 >= go2 + (a + 1 + k) ge2, the one piece-2 run from the same start;
//     equality in either needs go1 == ge2, hence ge2 == ge1 == go1: then piece 2 is dominated, E_2 <= E_1 in every cell, and the
//     term is inside E_1's own scan.
// F_p reads the true H of the row above.  No cell holds minus infinity (as in ssw_ends.hip), and the host's bound
// (m + n) max(|s|, go1, ge1, go2, ge2) < 2^30 keeps int32.  A chunk hands H, E_1 and E_2 of its last column on: three values per row.
// STORE: one byte per cell -- bits 0..2 H's source (0 diagonal, 1 E_1, 2 E_2, 3 F_1, 4 F_2; that order is the tie rule), bit 3
// "E_1 opened here", bit 4 "E_2 opened here", bit 5 "F_1 opened here", bit 6 "F_2 opened here" -- 8 bytes per lane and row, one
// 8-byte store; ssw_ends2_walk_kernel walks them back with pr_walk2 (ssw_pairs.h).  tests/twopiece_check.py is the definition.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "clh_device.h"
#include "clh_device_ops.h"
#include "ssw_pairs.h"

namespace clh {

static_assert(kEnCpl == 8, "a lane's row of decisions is two 32-bit words: 8 columns x 1 byte");

// minus the cost of one gap of j letters, j >= 1 (unsigned arithmetic: lanes past column n hold garbage, not UB)
__device__ __forceinline__ int en2_gap(int j, const En2Params& prm)
{
    const int a = (int)(0u - (uint32_t)prm.go - (uint32_t)(j - 1) * (uint32_t)prm.ge);
    const int b = (int)(0u - (uint32_t)prm.go2 - (uint32_t)(j - 1) * (uint32_t)prm.ge2);
    return pr_max(a, b);
}
template <int MODE>
__device__ __forceinline__ int en2_row0(int j, const En2Params& prm) { return (en_anchored(MODE) && j > 0) ? en2_gap(j, prm) : 0; }
template <int MODE>
__device__ __forceinline__ int en2_col0(int i, const En2Params& prm) { return (MODE == EN_OVERLAP || i == 0) ? 0 : en2_gap(i, prm); }

template <int MODE, bool STORE>
__global__ void __launch_bounds__(64) ssw_ends2_kernel(const En2Params prm, int first, int count)
{
    __shared__ int smat[32 * 32];                    // [query code][reference code]
    const int lane = threadIdx.x & 63;
    pr_load_matrix(smat, prm.mat, prm.n_mat, lane);
    const int x = (int)blockIdx.x;
    if (x >= count || first + x >= prm.npairs) return;
    const EnPair pr = prm.pairs[first + x];
    const int m = pr.m, n = pr.n;
    if (m <= 0 || n <= 0) return;                    // an empty side is answered by fetch
    const int go1 = prm.go, ge1 = prm.ge, go2 = prm.go2, ge2 = prm.ge2;
    const int nchunks = (n + kEnChunk - 1) / kEnChunk;
    const int mpad = (m + 63) & ~63;
    // hand-over buffers of this pair: [buffer 0 / 1][H / E_1 / E_2][mpad]
    if (nchunks > 1 && (pr.hand_off < 0 || pr.hand_off + (int64_t)6 * mpad > prm.hand_cap)) return;
    int32_t* hand = prm.hand + (nchunks > 1 ? pr.hand_off : 0);
    const int8_t* qry = prm.qry + pr.q_off;
    const int8_t* ref = prm.ref + pr.r_off;
    bool ws_ok = true;
    if (STORE) {
        const int llast = (n - (nchunks - 1) * kEnChunk + kEnCpl - 1) / kEnCpl;
        const int64_t need = (int64_t)8 * m * ((int64_t)64 * (nchunks - 1) + llast);
        ws_ok = pr.ws_off >= 0 && (pr.ws_off & 7) == 0 && pr.ws_off + need <= prm.ws_cap;
    }

    int row_best = en2_col0<MODE>(m, prm), row_j = 0;          // the last row's running maximum, smallest column
    int col_best = 0, col_i = 0, corner = 0;                   // the last column's (H[0][n] = 0 where it counts), smallest row; H[m][n]
    const int ln = ((n - 1) % kEnChunk) / kEnCpl, kn = ((n - 1) % kEnChunk) % kEnCpl;
    int ext_v = 0, ext_i = 0, ext_j = 0;                       // extend: the best cell this lane has seen, seeded with (0, 0)
    const int base1 = (int)((uint32_t)(lane * kEnCpl) * (uint32_t)ge1), base2 = (int)((uint32_t)(lane * kEnCpl) * (uint32_t)ge2);

    for (int c = 0; c < nchunks; ++c) {
        const int c0 = c * kEnChunk;
        const bool last = c == nchunks - 1;
        const int cols = last ? n - c0 : kEnChunk;
        const int L = (cols + kEnCpl - 1) / kEnCpl;            // lanes with a column
        int rcode[kEnCpl], off1[kEnCpl], off2[kEnCpl], Hp[kEnCpl], F1p[kEnCpl], F2p[kEnCpl];
#pragma unroll
        for (int k = 0; k < kEnCpl; ++k) {
            const int p = lane * kEnCpl + k, j = c0 + 1 + p;
            rcode[k] = j <= n ? ((int)ref[j - 1] & 31) : 0;
            off1[k] = (int)((uint32_t)(p + 1) * (uint32_t)ge1 - (uint32_t)go1);
            off2[k] = (int)((uint32_t)(p + 1) * (uint32_t)ge2 - (uint32_t)go2);
            Hp[k] = en2_row0<MODE>(j, prm);
            F1p[k] = Hp[k] - go1;
            F2p[k] = Hp[k] - go2;
        }
        int hleft = en2_row0<MODE>(c0 + lane * kEnCpl, prm);             // H[i-1][first own column - 1]
        const int32_t* inH = hand + (size_t)((c + 1) & 1) * 3 * mpad;    // written by chunk c - 1
        const int32_t* inE1 = inH + mpad;
        const int32_t* inE2 = inE1 + mpad;
        int32_t* outHp = hand + (size_t)(c & 1) * 3 * mpad;
        int32_t* outE1p = outHp + mpad;
        int32_t* outE2p = outE1p + mpad;
        uint2* wsp = nullptr;
        if (STORE && ws_ok) wsp = (uint2*)(prm.ws + pr.ws_off) + (size_t)c * m * 64;
        const int own = cols - lane * kEnCpl;                  // extend: register k holds a column of the reference while k < own
        int cv = (int)0x80000000, ci = 0, ck = 0;              // extend: this chunk's best of the lane

        for (int i0 = 0; i0 < m; i0 += 64) {
            const bool mine = i0 + lane < m;
            const int qv = mine ? ((int)qry[i0 + lane] & 31) : 0;
            int vH = 0, vE1 = 0, vE2 = 0, outH = 0, outE1 = 0, outE2 = 0;
            if (c > 0 && mine) { vH = inH[i0 + lane]; vE1 = inE1[i0 + lane]; vE2 = inE2[i0 + lane]; }
            const int rows = m - i0 < 64 ? m - i0 : 64;
            for (int rr = 0; rr < rows; ++rr) {
                const int i = i0 + rr + 1;
                const int qc = __builtin_amdgcn_readlane(qv, rr);
                int hin, E01, E02;                                       // H of the column in front of the chunk, E_p of the chunk's first column, this row
                if (c == 0) { hin = en2_col0<MODE>(i, prm); E01 = hin - go1; E02 = hin - go2; }
                else {
                    hin = __builtin_amdgcn_readlane(vH, rr);
                    E01 = pr_max(__builtin_amdgcn_readlane(vE1, rr) - ge1, hin - go1);
                    E02 = pr_max(__builtin_amdgcn_readlane(vE2, rr) - ge2, hin - go2);
                }
                const int* srow = smat + qc * 32;
                int T[kEnCpl], F1[kEnCpl], F2[kEnCpl], D[kEnCpl], H[kEnCpl], E1[kEnCpl], E2[kEnCpl];
                int v1 = 0, v2 = 0;
#pragma unroll
                for (int k = 0; k < kEnCpl; ++k) {
                    F1[k] = pr_max(Hp[k] - go1, F1p[k] - ge1);
                    F2[k] = pr_max(Hp[k] - go2, F2p[k] - ge2);
                    D[k] = (k ? Hp[k - 1] : hleft) + srow[rcode[k]];
                    T[k] = pr_max(pr_max(D[k], F1[k]), F2[k]);
                    const int x1 = T[k] + off1[k], x2 = T[k] + off2[k];
                    v1 = k ? pr_max(v1, x1) : x1;
                    v2 = k ? pr_max(v2, x2) : x2;
                }
                v1 = lane == 0 ? pr_max(v1, E01) : v1;
                v2 = lane == 0 ? pr_max(v2, E02) : v2;
                const int s1 = wave_prefix_max(v1), s2 = wave_prefix_max(v2);
                int e1 = dpp_shr1(E01, s1) - base1, e2 = dpp_shr1(E02, s2) - base2;      // lane 0 keeps E0_p (its base is 0)
#pragma unroll
                for (int k = 0; k < kEnCpl; ++k) {
                    E1[k] = e1; E2[k] = e2;
                    H[k] = pr_max(T[k], pr_max(e1, e2));
                    e1 = pr_max(e1 - ge1, T[k] - go1);
                    e2 = pr_max(e2 - ge2, T[k] - go2);
                }
                const int nleft = dpp_shr1(hin, H[kEnCpl - 1]);          // H[i][first own column - 1]
                if (STORE) {
                    uint32_t w[2] = {0u, 0u};
#pragma unroll
                    for (int k = 0; k < kEnCpl; ++k) {
                        const int left = k ? H[k - 1] : nleft;
                        const uint32_t src = H[k] == D[k] ? 0u : (H[k] == E1[k] ? 1u : (H[k] == E2[k] ? 2u : (H[k] == F1[k] ? 3u : 4u)));
                        const uint32_t b = src | (E1[k] == left - go1 ? 8u : 0u) | (E2[k] == left - go2 ? 16u : 0u) |
                                           (F1[k] == Hp[k] - go1 ? 32u : 0u) | (F2[k] == Hp[k] - go2 ? 64u : 0u);
                        w[k >> 2] |= b << (8 * (k & 3));
                    }
                    if (wsp && lane < L) wsp[(size_t)(i - 1) * L + lane] = make_uint2(w[0], w[1]);
                }
                if (!last) {
                    const int sH = __builtin_amdgcn_readlane(H[kEnCpl - 1], 63);
                    const int sE1 = __builtin_amdgcn_readlane(E1[kEnCpl - 1], 63), sE2 = __builtin_amdgcn_readlane(E2[kEnCpl - 1], 63);
                    outH = lane == rr ? sH : outH;                      // lane rr keeps row i0 + rr: one coalesced store per 64 rows
                    outE1 = lane == rr ? sE1 : outE1;
                    outE2 = lane == rr ? sE2 : outE2;
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
                        const int v2x = __shfl_xor(bv, d), j2 = __shfl_xor(bj, d);
                        const bool take = v2x > bv || (v2x == bv && j2 < bj);
                        bv = take ? v2x : bv; bj = take ? j2 : bj;
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
                for (int k = 0; k < kEnCpl; ++k) { Hp[k] = H[k]; F1p[k] = F1[k]; F2p[k] = F2[k]; }
                hleft = nleft;
            }
            if (!last && mine) { outHp[i0 + lane] = outH; outE1p[i0 + lane] = outE1; outE2p[i0 + lane] = outE2; }
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
            const int v2x = __shfl_xor(ext_v, d), i2 = __shfl_xor(ext_i, d), j2 = __shfl_xor(ext_j, d);
            const bool take = v2x > ext_v || (v2x == ext_v && (i2 < ext_i || (i2 == ext_i && j2 < ext_j)));
            ext_v = take ? v2x : ext_v; ext_i = take ? i2 : ext_i; ext_j = take ? j2 : ext_j;
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

// one lane per pair: pr_walk2 over the bytes the storing form left, chunk after chunk, per chunk row after row, 8 bytes per lane
__global__ void ssw_ends2_walk_kernel(const En2Params prm, int first, int count)
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
    const int64_t nbytes = (int64_t)8 * m * ((int64_t)64 * (nchunks - 1) + llast);
    if (pr.ws_off < 0 || pr.ws_off + nbytes > prm.ws_cap || pr.cig_off < 0 || pr.cig_off + pr.cig_cap > prm.cigar_cap) { row[7] = EN_ST_NO_WALK; return; }
    const uint8_t* ws = prm.ws + pr.ws_off;
    pr_walk2(row, prm.mode, m, n, prm.cigar + pr.cig_off, pr.cig_cap, [&](int i, int j) -> int {
        const int ch = (j - 1) / kEnChunk, p = (j - 1) % kEnChunk;
        const int L = ch == nchunks - 1 ? llast : 64;
        const int64_t bi = ((int64_t)ch * m * 64 + (int64_t)(i - 1) * L) * kEnCpl + p;
        if (bi < 0 || bi >= nbytes) return -1;
        return (int)ws[bi];
    });
}

template <int MODE>
static void en2_launch(const En2Params& p, bool store, int first, int count, hipStream_t st)
{
    if (store) hipLaunchKernelGGL((ssw_ends2_kernel<MODE, true>), dim3(count), dim3(64), 0, st, p, first, count);
    else hipLaunchKernelGGL((ssw_ends2_kernel<MODE, false>), dim3(count), dim3(64), 0, st, p, first, count);
}

hipError_t launch_ssw_ends2(const En2Params& p, bool store, int first, int count, hipStream_t stream)
{
    if (count <= 0) return hipSuccess;
    if (p.mode == EN_GLOBAL) en2_launch<EN_GLOBAL>(p, store, first, count, stream);
    else if (p.mode == EN_SEMIGLOBAL) en2_launch<EN_SEMIGLOBAL>(p, store, first, count, stream);
    else if (p.mode == EN_OVERLAP) en2_launch<EN_OVERLAP>(p, store, first, count, stream);
    else if (p.mode == EN_PREFIX) en2_launch<EN_PREFIX>(p, store, first, count, stream);
    else if (p.mode == EN_EXTEND) en2_launch<EN_EXTEND>(p, store, first, count, stream);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_ssw_ends2_walk(const En2Params& p, int first, int count, hipStream_t stream)
{
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(ssw_ends2_walk_kernel, dim3((count + 63) / 64), dim3(64), 0, stream, p, first, count);
    return hipGetLastError();
}

}  // namespace clh
