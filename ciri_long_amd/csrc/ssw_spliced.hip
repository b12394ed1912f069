// ssw_spliced.hip -- K1g with intron gaps: a maximal run of skipped reference letters r[a..b] costs min(go + (b - a) ge, io + start(a)
// + end(b)), the splice-site costs start / end read from the dinucleotides at the run's two ends on the pair's strand (gfx950).
//
// The sibling of ssw_ends_kernel (ssw_ends.hip) and ssw_ends2_kernel (ssw_ends2.hip), in a file of its own so that the one- and two-piece
// instantiations compile as they did: the same geometry (one wave per pair, kEnCpl columns per lane, chunks of kEnChunk columns), the
// same modes, boundaries, end cells and `extend`'s lane-private best cell.  With don(j) = start(j - 1) and acc(j) = end(j - 1) for the
// 1-based column j, per row step and lane:
//     F[k] = max(Hprev[k] - go, Fprev[k] - ge)                        lane-private; reads the true H
//     T[k] = max(diag[k] + s, F[k])                                   H without a reference gap
//     V    = max over k of T[k] - go + (p + 1) ge                     p = 8 lane + k; the max-plus scan of E as in ssw_ends2.hip
//     W    = max over k of T[k] - io - don(j + 1)                     the intron costs nothing per letter: a plain prefix maximum
//     e, u = exclusive prefix maxima of V and W over the lanes, lane 0 seeded with E and N of the chunk's first column
//     along the lane  E[k] = e,  N[k] = u,  H[k] = max(T[k], E[k], N[k] - acc(j)),  e = max(e - ge, T[k] - go),  u = max(u, T[k] - io - don(j + 1))
// E and N open from T, never from H: a deletion run and an intron run are never adjacent, which is what makes the one rule exact
// (tests/spliced_check.py is the definition).  io + don(j + 1) and acc(j) depend on the column alone and are set up once per chunk from
// the lane's own letters, one letter before and two after them; a dinucleotide with a code >= 4 or a letter off the reference costs
// `other`.  Both strands' tables lie in LDS as costs of the dinucleotide as the reference reads it (the host complements them for
// strand -).  A chunk hands T, E and N of its last column on, three values per row; the next chunk rebuilds that column's H = max(T,
// E, N - acc) for its first diagonal.  (H in place of T would let a deletion follow an intron, or an intron a deletion, across the
// chunk edge.)  Row 0 of the anchored modes is H[0][j] = -min(go + (j - 1) ge, io + don(1) + acc(j)).  No cell holds minus infinity: E
// and N of column 0 enter as one opening below T, which gives the same first E and N, and the host's bound (m + n) max(|s|, go, ge,
// io + dmax + amax) < 2^30 keeps int32.
// STORE: one byte per cell -- bits 0..1 H's source (0 diagonal, 1 E, 2 N, 3 F; that order is the tie rule), bit 2 T's source (0
// diagonal, 1 F), bit 3 "E opened here", bit 4 "N opened here", bit 5 "F opened here" -- 8 bytes per lane and row, one 8-byte store;
// ssw_spliced_walk_kernel walks them back with pr_walk_spliced (ssw_pairs.h).  tools/spliced_model.py is this scheme in Python.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "clh_device.h"
#include "clh_device_ops.h"
#include "ssw_pairs.h"

namespace clh {

static_assert(kEnCpl == 8, "a lane's row of decisions is two 32-bit words: 8 columns x 1 byte");

// the cost of the dinucleotide (x, y) as the reference reads it; site[0..15] start and site[16..31] end of the strand, site[kSpOther] other
__device__ __forceinline__ int sp_site(const int* site, int strand_off, int which, int x, int y)
{
    return site[((x | y) > 3) ? kSpOther : strand_off + which + 4 * x + y];
}

template <int MODE>
__device__ __forceinline__ int sp_col0(int i, int go, int ge)
{
    return (MODE == EN_OVERLAP || i == 0) ? 0 : (int)(0u - (uint32_t)go - (uint32_t)(i - 1) * (uint32_t)ge);
}
// H[0][j], j >= 1: 0 on a free row, else the cheaper of one deletion and one intron of j letters; iod1 = io + don(1), a = acc(j)
template <int MODE>
__device__ __forceinline__ int sp_row0(int j, int go, int ge, int iod1, int a)
{
    if (!en_anchored(MODE)) return 0;
    const int del = (int)((uint32_t)go + (uint32_t)(j - 1) * (uint32_t)ge), intron = iod1 + a;
    return -(del < intron ? del : intron);
}

template <int MODE, bool STORE>
__global__ void __launch_bounds__(64) ssw_spliced_kernel(const SpParams prm, int first, int count)
{
    __shared__ int smat[32 * 32];                    // [query code][reference code]
    __shared__ int site[kSpSites];
    const int lane = threadIdx.x & 63;
    for (int k = lane; k < kSpSites; k += 64) site[k] = prm.site[k];
    pr_load_matrix(smat, prm.mat, prm.n_mat, lane);  // ends on the barrier that also publishes `site`
    const int x = (int)blockIdx.x;
    if (x >= count || first + x >= prm.npairs) return;
    const EnPair pr = prm.pairs[first + x];
    const int m = pr.m, n = pr.n;
    if (m <= 0 || n <= 0) return;                    // an empty side is answered by fetch
    const int go = prm.go, ge = prm.ge, io = prm.io;
    const int soff = (prm.strand && prm.strand[first + x] < 0) ? 32 : 0;
    const int nchunks = (n + kEnChunk - 1) / kEnChunk;
    const int mpad = (m + 63) & ~63;
    // hand-over buffers of this pair: [buffer 0 / 1][T / E / N][mpad]
    if (nchunks > 1 && (pr.hand_off < 0 || pr.hand_off + (int64_t)6 * mpad > prm.hand_cap)) return;
    int32_t* hand = prm.hand + (nchunks > 1 ? pr.hand_off : 0);
    const int8_t* qry = prm.qry + pr.q_off;
    const int8_t* ref = prm.ref + pr.r_off;
    auto letter = [&](int pos) -> int { return (pos >= 0 && pos < n) ? ((int)ref[pos] & 31) : 4; };      // 0-based; 4 off the reference
    bool ws_ok = true;
    if (STORE) {
        const int llast = (n - (nchunks - 1) * kEnChunk + kEnCpl - 1) / kEnCpl;
        const int64_t need = (int64_t)8 * m * ((int64_t)64 * (nchunks - 1) + llast);
        ws_ok = pr.ws_off >= 0 && (pr.ws_off & 7) == 0 && pr.ws_off + need <= prm.ws_cap;
    }

    int row_best = sp_col0<MODE>(m, go, ge), row_j = 0;        // the last row's running maximum, smallest column
    int col_best = 0, col_i = 0, corner = 0;                   // the last column's (H[0][n] = 0 where it counts), smallest row; H[m][n]
    const int ln = ((n - 1) % kEnChunk) / kEnCpl, kn = ((n - 1) % kEnChunk) % kEnCpl;
    int ext_v = 0, ext_i = 0, ext_j = 0;                       // extend: the best cell this lane has seen, seeded with (0, 0)
    const int base = (int)((uint32_t)(lane * kEnCpl) * (uint32_t)ge);
    const int iod1 = io + sp_site(site, soff, 0, letter(0), letter(1));      // io + don(1)

    for (int c = 0; c < nchunks; ++c) {
        const int c0 = c * kEnChunk;
        const bool last = c == nchunks - 1;
        const int cols = last ? n - c0 : kEnChunk;
        const int L = (cols + kEnCpl - 1) / kEnCpl;            // lanes with a column
        // what the column in front of the chunk needs: io + don(c0 + 1), acc(c0) and H[0][c0]
        const int iod_in = io + sp_site(site, soff, 0, letter(c0), letter(c0 + 1));
        const int acc_in = sp_site(site, soff, 16, letter(c0 - 2), letter(c0 - 1));
        const int h0_in = c0 ? sp_row0<MODE>(c0, go, ge, iod1, acc_in) : 0;
        int lt[kEnCpl + 3];                                     // the letters of columns j - 1 .. j + 9 of the lane's first column j
#pragma unroll
        for (int t = 0; t < kEnCpl + 3; ++t) lt[t] = letter(c0 + lane * kEnCpl - 1 + t);
        int rcode[kEnCpl], off[kEnCpl], iod[kEnCpl], acc[kEnCpl], Hp[kEnCpl], Fp[kEnCpl];
#pragma unroll
        for (int k = 0; k < kEnCpl; ++k) {
            const int p = lane * kEnCpl + k, j = c0 + 1 + p;
            rcode[k] = j <= n ? lt[k + 1] : 0;
            off[k] = (int)((uint32_t)(p + 1) * (uint32_t)ge - (uint32_t)go);
            iod[k] = io + sp_site(site, soff, 0, lt[k + 2], lt[k + 3]);      // io + don(j + 1): what opening an intron behind column j costs
            acc[k] = sp_site(site, soff, 16, lt[k], lt[k + 1]);             // acc(j)
            Hp[k] = sp_row0<MODE>(j, go, ge, iod1, acc[k]);
            Fp[k] = Hp[k] - go;
        }
        int hleft = dpp_shr1(h0_in, Hp[kEnCpl - 1]);                      // H[i-1][first own column - 1]
        const int32_t* inT = hand + (size_t)((c + 1) & 1) * 3 * mpad;    // written by chunk c - 1
        const int32_t* inE = inT + mpad;
        const int32_t* inN = inE + mpad;
        int32_t* outTp = hand + (size_t)(c & 1) * 3 * mpad;
        int32_t* outEp = outTp + mpad;
        int32_t* outNp = outEp + mpad;
        uint2* wsp = nullptr;
        if (STORE && ws_ok) wsp = (uint2*)(prm.ws + pr.ws_off) + (size_t)c * m * 64;
        const int own = cols - lane * kEnCpl;                  // extend: register k holds a column of the reference while k < own
        int cv = (int)0x80000000, ci = 0, ck = 0;              // extend: this chunk's best of the lane

        for (int i0 = 0; i0 < m; i0 += 64) {
            const bool mine = i0 + lane < m;
            const int qv = mine ? ((int)qry[i0 + lane] & 31) : 0;
            int vT = 0, vE = 0, vN = 0, outT = 0, outE = 0, outN = 0;
            if (c > 0 && mine) { vT = inT[i0 + lane]; vE = inE[i0 + lane]; vN = inN[i0 + lane]; }
            const int rows = m - i0 < 64 ? m - i0 : 64;
            for (int rr = 0; rr < rows; ++rr) {
                const int i = i0 + rr + 1;
                const int qc = __builtin_amdgcn_readlane(qv, rr);
                int tin, hin, E0, N0;                          // T and H of the column in front of the chunk, E and N of the chunk's first column, this row
                if (c == 0) { tin = sp_col0<MODE>(i, go, ge); hin = tin; E0 = tin - go; N0 = tin - iod_in; }
                else {
                    tin = __builtin_amdgcn_readlane(vT, rr);
                    const int ein = __builtin_amdgcn_readlane(vE, rr), nin = __builtin_amdgcn_readlane(vN, rr);
                    hin = pr_max(tin, pr_max(ein, nin - acc_in));
                    E0 = pr_max(ein - ge, tin - go);
                    N0 = pr_max(nin, tin - iod_in);
                }
                const int* srow = smat + qc * 32;
                int T[kEnCpl], F[kEnCpl], D[kEnCpl], H[kEnCpl], E[kEnCpl], N[kEnCpl], X[kEnCpl];
                int ve = 0, vn = 0;
#pragma unroll
                for (int k = 0; k < kEnCpl; ++k) {
                    F[k] = pr_max(Hp[k] - go, Fp[k] - ge);
                    D[k] = (k ? Hp[k - 1] : hleft) + srow[rcode[k]];
                    T[k] = pr_max(D[k], F[k]);
                    X[k] = T[k] - iod[k];
                    const int xe = T[k] + off[k];
                    ve = k ? pr_max(ve, xe) : xe;
                    vn = k ? pr_max(vn, X[k]) : X[k];
                }
                ve = lane == 0 ? pr_max(ve, E0) : ve;
                vn = lane == 0 ? pr_max(vn, N0) : vn;
                const int se = wave_prefix_max(ve), sn = wave_prefix_max(vn);
                int e = dpp_shr1(E0, se) - base, u = dpp_shr1(N0, sn);   // lane 0 keeps E0 (its base is 0) and N0
#pragma unroll
                for (int k = 0; k < kEnCpl; ++k) {
                    E[k] = e; N[k] = u;
                    H[k] = pr_max(T[k], pr_max(e, u - acc[k]));
                    e = pr_max(e - ge, T[k] - go);
                    u = pr_max(u, X[k]);
                }
                const int nleft = dpp_shr1(hin, H[kEnCpl - 1]);          // H[i][first own column - 1]
                if (STORE) {
                    const int tleft = dpp_shr1(tin, T[kEnCpl - 1]);      // T[i][first own column - 1]
                    const int xleft = dpp_shr1(tin - iod_in, X[kEnCpl - 1]);
                    uint32_t w[2] = {0u, 0u};
#pragma unroll
                    for (int k = 0; k < kEnCpl; ++k) {
                        const int tl = k ? T[k - 1] : tleft, xl = k ? X[k - 1] : xleft;
                        const uint32_t src = H[k] == D[k] ? 0u : (H[k] == E[k] ? 1u : (H[k] == N[k] - acc[k] ? 2u : 3u));
                        const uint32_t b = src | (T[k] == D[k] ? 0u : 4u) | (E[k] == tl - go ? 8u : 0u) | (N[k] == xl ? 16u : 0u) |
                                           (F[k] == Hp[k] - go ? 32u : 0u);
                        w[k >> 2] |= b << (8 * (k & 3));
                    }
                    if (wsp && lane < L) wsp[(size_t)(i - 1) * L + lane] = make_uint2(w[0], w[1]);
                }
                if (!last) {
                    const int sT = __builtin_amdgcn_readlane(T[kEnCpl - 1], 63);
                    const int sE = __builtin_amdgcn_readlane(E[kEnCpl - 1], 63), sN = __builtin_amdgcn_readlane(N[kEnCpl - 1], 63);
                    outT = lane == rr ? sT : outT;                      // lane rr keeps row i0 + rr: one coalesced store per 64 rows
                    outE = lane == rr ? sE : outE;
                    outN = lane == rr ? sN : outN;
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
            if (!last && mine) { outTp[i0 + lane] = outT; outEp[i0 + lane] = outE; outNp[i0 + lane] = outN; }
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

// one lane per pair: pr_walk_spliced over the bytes the storing form left, chunk after chunk, per chunk row after row, 8 bytes per lane,
// read 8 at a time: an intron is thousands of steps along one row, and each of its words is loaded once
__global__ void ssw_spliced_walk_kernel(const SpParams prm, int first, int count)
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
    if (pr.ws_off < 0 || (pr.ws_off & 7) != 0 || pr.ws_off + nbytes > prm.ws_cap || pr.cig_off < 0 || pr.cig_off + pr.cig_cap > prm.cigar_cap) { row[7] = EN_ST_NO_WALK; return; }
    const uint2* ws = (const uint2*)(prm.ws + pr.ws_off);        // a lane's 8 bytes of a row; nbytes is a multiple of 8
    int64_t held = -1;                                           // the word the last step read: a run along a row reads each once
    uint2 word = make_uint2(0u, 0u);
    const int8_t* ref = prm.ref + pr.r_off;
    const int soff = (prm.strand && prm.strand[first + x] < 0) ? 32 : 0;
    auto letter = [&](int pos) -> int { return (pos >= 0 && pos < n) ? ((int)ref[pos] & 31) : 4; };
    pr_walk_spliced(row, prm.mode, m, n, prm.cigar + pr.cig_off, pr.cig_cap,
        [&](int i, int j) -> int {
            const int ch = (j - 1) / kEnChunk, p = (j - 1) % kEnChunk;
            const int L = ch == nchunks - 1 ? llast : 64;
            const int64_t wi = (int64_t)ch * m * 64 + (int64_t)(i - 1) * L + p / kEnCpl;
            if (wi < 0 || wi * 8 + 8 > nbytes) return -1;
            if (wi != held) { word = ws[wi]; held = wi; }
            return (int)((((p & 4) ? word.y : word.x) >> (8 * (p & 3))) & 255u);
        },
        [&](int i, int j, uint32_t bit, bool* opened) -> int {      // the cells of the run from (i, j) leftwards inside the lane's word
            const int ch = (j - 1) / kEnChunk, p = (j - 1) % kEnChunk, k = p % kEnCpl;
            const int L = ch == nchunks - 1 ? llast : 64;
            const int64_t wi = (int64_t)ch * m * 64 + (int64_t)(i - 1) * L + p / kEnCpl;
            if (wi < 0 || wi * 8 + 8 > nbytes) return 0;
            if (wi != held) { word = ws[wi]; held = wi; }
            const uint64_t both = ((uint64_t)word.y << 32) | word.x;
            const uint64_t set = both & (0x0101010101010101ull * bit) & (~0ull >> (8 * (7 - k)));      // "opened here" of columns 0 .. k of the word
            *opened = set != 0;
            return set ? k - (63 - __builtin_clzll(set)) / 8 + 1 : k + 1;
        },
        [&](int j) -> int {      // the run of j letters on row 0: D (2) if the deletion is not dearer, else N (3)
            const int64_t del = (int64_t)prm.go + (int64_t)(j - 1) * prm.ge;
            const int64_t intron = (int64_t)prm.io + sp_site(prm.site, soff, 0, letter(0), letter(1)) + sp_site(prm.site, soff, 16, letter(j - 2), letter(j - 1));
            return del <= intron ? 2 : 3;
        });
}

template <int MODE>
static void sp_launch(const SpParams& p, bool store, int first, int count, hipStream_t st)
{
    if (store) hipLaunchKernelGGL((ssw_spliced_kernel<MODE, true>), dim3(count), dim3(64), 0, st, p, first, count);
    else hipLaunchKernelGGL((ssw_spliced_kernel<MODE, false>), dim3(count), dim3(64), 0, st, p, first, count);
}

hipError_t launch_ssw_spliced(const SpParams& p, bool store, int first, int count, hipStream_t stream)
{
    if (count <= 0) return hipSuccess;
    if (p.mode == EN_GLOBAL) sp_launch<EN_GLOBAL>(p, store, first, count, stream);
    else if (p.mode == EN_SEMIGLOBAL) sp_launch<EN_SEMIGLOBAL>(p, store, first, count, stream);
    else if (p.mode == EN_OVERLAP) sp_launch<EN_OVERLAP>(p, store, first, count, stream);
    else if (p.mode == EN_PREFIX) sp_launch<EN_PREFIX>(p, store, first, count, stream);
    else if (p.mode == EN_EXTEND) sp_launch<EN_EXTEND>(p, store, first, count, stream);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_ssw_spliced_walk(const SpParams& p, int first, int count, hipStream_t stream)
{
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(ssw_spliced_walk_kernel, dim3((count + 63) / 64), dim3(64), 0, stream, p, first, count);
    return hipGetLastError();
}

}  // namespace clh
