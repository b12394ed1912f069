// ssw_band.hip -- K1gb: K1g's global, semiglobal, prefix and extend programmes over a band of diagonals, in the band's own frame (gfx950).
//
// The band of a pair is [lo, hi] in d = j - i (i query letters, j reference letters), B = hi - lo + 1 <= 64 CPL diagonals.  One wave
// takes one pair; lane l owns the CPL consecutive band positions b = d - lo = l CPL + k, the loop runs over the query rows, and
// position b of row i is the cell (i, i + lo + b).  In this frame
//     the diagonal source (i-1, j-1) is the lane's own cell of the row before,
//     F's source (i-1, j) is position b + 1 of the row before: the next register, or the next lane's first (one wave_shl:1 move),
//     E along the row is K1g's max-plus prefix scan in the frame E[p] + p ge (wave_prefix_max, one exclusive shift, CPL steps),
// and nothing but the LDS matrix lies outside registers: the band is one chunk, there is no hand-over.  Per row step and lane:
//     F[k] = max(Hprev[k+1] - go, Fprev[k+1] - ge)
//     T[k] = max(Hprev[k] + s, F[k])                                  H without E
//     X[k] = T[k] - go + (p + 1) ge  where the cell exists, else minus infinity;   V = max over k of X[k]
//     u    = exclusive prefix maximum of V over the lanes, seeded with minus infinity
//     E[k] = u - p ge,  H[k] = max(T[k], E[k]) where the cell exists, else minus infinity,  u = max(u, X[k])
// A position is a cell of row i while 0 <= j <= n (and b < B): the cells of column 0 and of column n move through the positions as
// the rows go, which is one unsigned comparison of the position's column counter per cell and selects, never a branch.  Column 0
// needs nothing else: its cell has no diagonal source (the position held minus infinity in the row before) and no E, so H = F, the
// gap from (0, 0), exactly while the band holds the cells above it.  Row 0 is written into the registers before the loop.  The
// reference letter of a position moves by one per row: the letters slide down the positions with the rows (a register window, one
// wave_shl:1 move per row), and the letter that enters at the top comes from a register loaded once per 64 rows (v_readlane), as
// the query letter does.
// Minus infinity is kBdNeg (clh_device.h has the bound that keeps it apart from every score).  Every cell of an admitted band is
// reached from a start cell, so H and T of a cell are scores; E and F may be minus infinity, and then they equal no H.
// prefix and extend have global's row 0; prefix ends where semiglobal does, over the band's cells of row m.  extend ends at the
// greatest H over the band's cells, smallest i, then smallest j: a lane keeps the best of its own cells under a bare > (rows ascend,
// and a lane's columns ascend within a row), seeded with (0, (0, 0)), which cells of column 0 (<= 0) and positions that are no cell
// (minus infinity) never beat, and the lanes are reduced once by the key after the last row.
// STORE: 4 bits per cell as in K1g (H's source 0 diagonal / 1 E / 2 F, "E opened here", "F opened here"), CPL / 2 bytes per lane and
// row, only the lanes that own a band position: m ceil(B / CPL) CPL / 2 bytes per pair.  ssw_band_walk_kernel<Prm> walks them back, one
// lane per pair: a diagonal step keeps b, a D step goes to b - 1, an I step to b + 1.  The walk itself is K1g's, pr_walk<MODEL> in
// ssw_pairs.h, and BdCells there says where the half-byte or byte of a cell lies.
// tools/band_model.py is this scheme in Python for any geometry; tests/band_check.py is the definition.
//
// Two pieces (Bd2Params): a gap of k letters costs min(go + (k - 1) ge, go2 + (k - 1) ge2); go / ge / E / F are piece 1 and go2 / ge2
// / E2 / F2 piece 2.  The gap model is a constant derived from the parameter block and ssw_band_kernel is one body for both: piece
// 2's statements stand under `if constexpr` next to piece 1's, in the same frame, with the same classes of 2, 4 and 8 positions per
// lane, the same modes, end cells, tie rules and minus infinity, and no device helper in or around the row loop.  Per
// row step and lane:
//     F_p[k] = max(Hprev[k+1] - go_p, F_pprev[k+1] - ge_p)            p = 1, 2 (one wave_shl:1 move per piece and for H)
//     T[k]   = max(Hprev[k] + s, F_1[k], F_2[k])                      H without E
//     X_p[k] = T[k] - go_p + (b + 1) ge_p  where the cell exists, else minus infinity;   V_p = max over k of X_p[k]
//     u_p    = exclusive prefix maximum of V_p over the lanes, seeded with minus infinity: two independent wave_prefix_max chains
//     E_p[k] = u_p - b ge_p,  H[k] = max(T[k], E_1[k], E_2[k]) where the cell exists, else minus infinity,  u_p = max(u_p, X_p[k])
// The scan of piece p does not see the other piece's E through H; under 0 <= ge2 <= ge1 <= go1 <= go2 that changes nothing the walk
// reads (the argument is in ssw_ends.hip; a band only removes cells).  The host's bound takes the maximum over all four costs.
// STORE: one byte per cell -- bits 0..2 H's source (0 diagonal, 1 E_1, 2 E_2, 3 F_1, 4 F_2; that order is the tie rule), bits 3..6
// "opened here" of E_1, E_2, F_1, F_2 -- CPL bytes per lane and row, only the lanes that own a band position: m ceil(B / CPL) CPL bytes
// per pair.  tests/twopiece_check.py is the definition.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "clh_device.h"
#include "clh_device_ops.h"
#include "ssw_pairs.h"

namespace clh {

// the gap model of a parameter block, and a lane's row of decisions: CPL cells of 4 bits (one piece) or 8 (two pieces)
template <typename Prm> struct BdModel;
template <> struct BdModel<BdParams> { static constexpr bool two = false; static constexpr int bits = 4; };
template <> struct BdModel<Bd2Params> { static constexpr bool two = true; static constexpr int bits = 8; };
template <int BYTES> struct BdWord;
template <> struct BdWord<1> { typedef uint8_t type; };
template <> struct BdWord<2> { typedef uint16_t type; };
template <> struct BdWord<4> { typedef uint32_t type; };
template <> struct BdWord<8> { typedef uint64_t type; };

__device__ __forceinline__ int bd_min(int a, int b) { return a < b ? a : b; }

template <typename Prm, int CPL, int MODE, bool STORE>
__global__ void __launch_bounds__(64) ssw_band_kernel(const Prm prm, int first, int count)
{
    constexpr bool two = BdModel<Prm>::two;
    constexpr int WB = CPL * BdModel<Prm>::bits / 8;                    // bytes of a lane's row of decisions
    typedef typename BdWord<WB>::type word_t;
    constexpr int W = 64 * CPL;
    __shared__ int smat[32 * 32];                    // [query code][reference code]
    const int lane = threadIdx.x & 63;
    pr_load_matrix(smat, prm.mat, prm.n_mat, lane);
    const int x = (int)blockIdx.x;
    if (x >= count || first + x >= prm.norder) return;
    const int pi = prm.order[first + x];
    if (pi < 0 || pi >= prm.npairs) return;
    const BdPair pr = prm.pairs[pi];
    const int m = pr.m, n = pr.n, lo = pr.lo;
    const int B = pr.hi - pr.lo + 1;
    // a pair the plan would not have filed here leaves its row unwritten, which fetch reports
    if (m <= 0 || n <= 0 || B < 1 || B > W || lo < -m || pr.hi > n) return;
    const int go = prm.go, ge = prm.ge;
    int go2 = 0, ge2 = 0;
    if constexpr (two) { go2 = prm.go2; ge2 = prm.ge2; }
    const int8_t* qry = prm.qry + pr.q_off;
    const int8_t* ref = prm.ref + pr.r_off;
    const int L = (B + CPL - 1) / CPL;               // lanes with a band position
    const int64_t rowbytes = (int64_t)L * WB;
    bool ws_ok = true;
    if (STORE) ws_ok = pr.ws_off >= 0 && (pr.ws_off & 15) == 0 && pr.ws_off + (int64_t)m * rowbytes <= prm.ws_cap;
    uint8_t* wsp = (STORE && ws_ok) ? prm.ws + pr.ws_off + (size_t)lane * WB : nullptr;

    int rc[CPL], jr[CPL], off[CPL], poff[CPL], Hp[CPL], Fp[CPL];
    int off2[CPL], poff2[CPL], F2p[CPL];                       // two pieces
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
        const int p = lane * CPL + k, j0 = lo + p;             // the position's column in row 0
        jr[k] = p < B ? j0 + 1 : 0x40000000;                   // its column in the row at hand; a position outside the band never is a cell
        rc[k] = (j0 >= 0 && j0 < n) ? ((int)ref[j0] & 31) : 0; // the letter of column j0 + 1, whatever B: it slides down to the band
        poff[k] = (int)((uint32_t)p * (uint32_t)ge);
        off[k] = (int)((uint32_t)(p + 1) * (uint32_t)ge - (uint32_t)go);
        if constexpr (two) {
            poff2[k] = (int)((uint32_t)p * (uint32_t)ge2);
            off2[k] = (int)((uint32_t)(p + 1) * (uint32_t)ge2 - (uint32_t)go2);
        }
        const bool cell = p < B && j0 >= 0 && j0 <= n;
        int h0;                                                // minus what one gap of j0 letters costs, where row 0 is anchored
        if constexpr (two) h0 = (en_anchored(MODE) && j0 > 0) ? -bd_min(go + (j0 - 1) * ge, go2 + (j0 - 1) * ge2) : 0;
        else h0 = (en_anchored(MODE) && j0 > 0) ? -(go + (j0 - 1) * ge) : 0;
        Hp[k] = cell ? h0 : kBdNeg;
        Fp[k] = kBdNeg;
        if constexpr (two) F2p[k] = kBdNeg;
    }
    const int bn = n - m - lo;                                 // the position of (m, n) in row m
    if (MODE == EN_GLOBAL && (bn < 0 || bn >= B)) return;
    const int ln = bn / CPL, kn = bn % CPL;
    int corner = kBdNeg, best_v = MODE == EN_EXTEND ? 0 : (int)0x80000000, best_i = 0, best_j = MODE == EN_EXTEND ? 0 : 0x7fffffff;

    for (int i0 = 0; i0 < m; i0 += 64) {
        const bool mine = i0 + lane < m;
        const int qv = mine ? ((int)qry[i0 + lane] & 31) : 0;
        const int64_t ridx = (int64_t)lo + W + i0 + lane;      // what enters at the top position after row i0 + lane + 1
        const int rv = (ridx >= 0 && ridx < n) ? ((int)ref[ridx] & 31) : 0;
        const int rows = m - i0 < 64 ? m - i0 : 64;
        for (int rr = 0; rr < rows; ++rr) {
            const int i = i0 + rr + 1;
            const int qc = __builtin_amdgcn_readlane(qv, rr);
            const int enter = __builtin_amdgcn_readlane(rv, rr);
            const int hnext = dpp_shl1(kBdNeg, Hp[0]), fnext = dpp_shl1(kBdNeg, Fp[0]);
            int f2next = 0;
            if constexpr (two) f2next = dpp_shl1(kBdNeg, F2p[0]);
            const int* srow = smat + qc * 32;
            int T[CPL], F[CPL], D[CPL], H[CPL], E[CPL], X[CPL], Hu[CPL];
            int F2[CPL], E2[CPL], X2[CPL];                     // two pieces
            bool ok[CPL];
            int v = kBdNeg, v2 = kBdNeg;
#pragma unroll
            for (int k = 0; k < CPL; ++k) {
                Hu[k] = k + 1 < CPL ? Hp[k + 1] : hnext;
                const int fu = k + 1 < CPL ? Fp[k + 1] : fnext;
                F[k] = pr_max(Hu[k] - go, fu - ge);
                if constexpr (two) F2[k] = pr_max(Hu[k] - go2, (k + 1 < CPL ? F2p[k + 1] : f2next) - ge2);
                D[k] = Hp[k] + srow[rc[k]];
                ok[k] = (uint32_t)jr[k] <= (uint32_t)n;
                if constexpr (two) T[k] = pr_max(pr_max(D[k], F[k]), F2[k]);
                else T[k] = pr_max(D[k], F[k]);
                X[k] = ok[k] ? T[k] + off[k] : kBdNeg;
                if constexpr (two) X2[k] = ok[k] ? T[k] + off2[k] : kBdNeg;
                v = pr_max(v, X[k]);
                if constexpr (two) v2 = pr_max(v2, X2[k]);
            }
            const int s = wave_prefix_max(v);
            int s2 = 0;
            if constexpr (two) s2 = wave_prefix_max(v2);
            int u = dpp_shr1(kBdNeg, s), u2 = 0;
            if constexpr (two) u2 = dpp_shr1(kBdNeg, s2);
#pragma unroll
            for (int k = 0; k < CPL; ++k) {
                E[k] = u - poff[k];
                if constexpr (two) {
                    E2[k] = u2 - poff2[k];
                    H[k] = ok[k] ? pr_max(T[k], pr_max(E[k], E2[k])) : kBdNeg;
                } else H[k] = ok[k] ? pr_max(T[k], E[k]) : kBdNeg;
                u = pr_max(u, X[k]);
                if constexpr (two) u2 = pr_max(u2, X2[k]);
            }
            if (STORE) {
                const int nleft = dpp_shr1(kBdNeg, H[CPL - 1]);          // H of position b - 1 of this row
                typename BdWord<two ? 8 : 4>::type w = 0;
#pragma unroll
                for (int k = 0; k < CPL; ++k) {
                    const int left = k ? H[k - 1] : nleft;
                    if constexpr (two) {
                        const uint32_t src = H[k] == D[k] ? 0u : (H[k] == E[k] ? 1u : (H[k] == E2[k] ? 2u : (H[k] == F[k] ? 3u : 4u)));
                        const uint32_t b = src | (E[k] == left - go ? 8u : 0u) | (E2[k] == left - go2 ? 16u : 0u) |
                                           (F[k] == Hu[k] - go ? 32u : 0u) | (F2[k] == Hu[k] - go2 ? 64u : 0u);
                        w |= (uint64_t)b << (8 * k);
                    } else {
                        const uint32_t src = H[k] == D[k] ? 0u : (H[k] == E[k] ? 1u : 2u);
                        const uint32_t nib = src | (E[k] == left - go ? 4u : 0u) | (F[k] == Hu[k] - go ? 8u : 0u);
                        w |= nib << (4 * k);
                    }
                }
                if (wsp && lane < L) *(word_t*)(wsp + (size_t)(i - 1) * rowbytes) = (word_t)w;
            }
            if (MODE == EN_EXTEND) {
#pragma unroll
                for (int k = 0; k < CPL; ++k)
                    if (H[k] > best_v) { best_v = H[k]; best_i = i; best_j = jr[k]; }
            } else if (i == m) {
                if (MODE == EN_GLOBAL) {
                    int hn = H[0];
#pragma unroll
                    for (int k = 1; k < CPL; ++k) hn = k == kn ? H[k] : hn;
                    corner = hn;                                         // meaningful in lane ln
                } else {
#pragma unroll
                    for (int k = 0; k < CPL; ++k)
                        if (ok[k] && H[k] > best_v) { best_v = H[k]; best_j = jr[k]; }
                }
            }
            const int r0 = rc[0];
#pragma unroll
            for (int k = 0; k < CPL; ++k) {
                Hp[k] = H[k]; Fp[k] = F[k];
                if constexpr (two) F2p[k] = F2[k];
                jr[k] += 1;
                if (k + 1 < CPL) rc[k] = rc[k + 1];
            }
            rc[CPL - 1] = dpp_shl1(enter, r0);
        }
    }
    int score, ej, ei = m;
    if (MODE == EN_GLOBAL) {
        score = __shfl(corner, ln); ej = n;
    } else if (MODE == EN_EXTEND) {
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int v2 = __shfl_xor(best_v, d), i2 = __shfl_xor(best_i, d), j2 = __shfl_xor(best_j, d);
            const bool take = v2 > best_v || (v2 == best_v && (i2 < best_i || (i2 == best_i && j2 < best_j)));
            best_v = take ? v2 : best_v; best_i = take ? i2 : best_i; best_j = take ? j2 : best_j;
        }
        score = best_v; ei = best_i; ej = best_j;
    } else {
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int v2 = __shfl_xor(best_v, d), j2 = __shfl_xor(best_j, d);
            const bool take = v2 > best_v || (v2 == best_v && j2 < best_j);
            best_v = take ? v2 : best_v; best_j = take ? j2 : best_j;
        }
        score = best_v; ej = best_j;
    }
    if (lane == 0) {
        int32_t* row = prm.rows + (size_t)pi * 8;
        row[0] = score;
        row[1] = en_anchored(MODE) ? 0 : -1;                      // begins: the walk's, unless the mode fixes them
        row[2] = ej - 1;
        row[3] = 0;
        row[4] = ei - 1;
        row[5] = 0;
        row[6] = 0;
        row[7] = (STORE && !ws_ok) ? EN_ST_NO_WALK : 0;
    }
}

// one lane per pair: pr_walk over the half-bytes or bytes the storing form left, where BdCells says they lie
template <typename Prm>
__global__ void ssw_band_walk_kernel(const Prm prm, int first, int count)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= count || first + x >= prm.npairs) return;
    const BdPair pr = prm.pairs[first + x];
    const int m = pr.m, n = pr.n;
    if (m <= 0 || n <= 0) return;
    int32_t* row = prm.rows + (size_t)(first + x) * 8;
    if (row[7] != 0) return;                                     // unwritten, or without stored decisions: fetch reports it
    const int B = pr.hi - pr.lo + 1;
    static_assert(kBdCpl[0] == 2 && kBdCpl[1] == 4 && kBdCpl[2] == 8, "the class index is log2(CPL) - 1");
    if (pr.cls < 0 || pr.cls >= kBdClasses) { row[7] = EN_ST_NO_WALK; return; }
    const int cpl = 2 << pr.cls;
    if (B < 1 || B > 64 * cpl) { row[7] = EN_ST_NO_WALK; return; }
    BdCells<BdModel<Prm>::bits> cells(m, pr.lo, B, cpl);
    if (pr.ws_off < 0 || pr.ws_off + cells.bytes() > prm.ws_cap || pr.cig_off < 0 || pr.cig_off + pr.cig_cap > prm.cigar_cap) { row[7] = EN_ST_NO_WALK; return; }
    cells.ws = prm.ws + pr.ws_off;
    pr_walk<BdModel<Prm>::two ? EN_TWO_PIECE : EN_ONE_PIECE>(row, prm.mode, m, n, prm.cigar + pr.cig_off, pr.cig_cap, cells);
}

template <typename Prm, int CPL, int MODE>
static void bd_launch_mode(const Prm& p, bool store, int first, int count, hipStream_t st)
{
    if (store) hipLaunchKernelGGL((ssw_band_kernel<Prm, CPL, MODE, true>), dim3(count), dim3(64), 0, st, p, first, count);
    else hipLaunchKernelGGL((ssw_band_kernel<Prm, CPL, MODE, false>), dim3(count), dim3(64), 0, st, p, first, count);
}

template <typename Prm, int CPL>
static void bd_launch_class(const Prm& p, bool store, int first, int count, hipStream_t st)
{
    if (p.mode == EN_GLOBAL) bd_launch_mode<Prm, CPL, EN_GLOBAL>(p, store, first, count, st);
    else if (p.mode == EN_PREFIX) bd_launch_mode<Prm, CPL, EN_PREFIX>(p, store, first, count, st);
    else if (p.mode == EN_EXTEND) bd_launch_mode<Prm, CPL, EN_EXTEND>(p, store, first, count, st);
    else bd_launch_mode<Prm, CPL, EN_SEMIGLOBAL>(p, store, first, count, st);
}

template <typename Prm>
static hipError_t bd_launch(const Prm& p, int cls, bool store, int first, int count, hipStream_t stream)
{
    if (count <= 0) return hipSuccess;
    if (p.mode != EN_GLOBAL && p.mode != EN_SEMIGLOBAL && p.mode != EN_PREFIX && p.mode != EN_EXTEND) return hipErrorInvalidValue;
    if (cls == 0) bd_launch_class<Prm, 2>(p, store, first, count, stream);
    else if (cls == 1) bd_launch_class<Prm, 4>(p, store, first, count, stream);
    else if (cls == 2) bd_launch_class<Prm, 8>(p, store, first, count, stream);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

template <typename Prm>
static hipError_t bd_launch_walk(const Prm& p, int first, int count, hipStream_t stream)
{
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(ssw_band_walk_kernel<Prm>, dim3((count + 63) / 64), dim3(64), 0, stream, p, first, count);
    return hipGetLastError();
}

hipError_t launch_ssw_band(const BdParams& p, int cls, bool store, int first, int count, hipStream_t stream) { return bd_launch(p, cls, store, first, count, stream); }
hipError_t launch_ssw_band2(const Bd2Params& p, int cls, bool store, int first, int count, hipStream_t stream) { return bd_launch(p, cls, store, first, count, stream); }
hipError_t launch_ssw_band_walk(const BdParams& p, int first, int count, hipStream_t stream) { return bd_launch_walk(p, first, count, stream); }
hipError_t launch_ssw_band2_walk(const Bd2Params& p, int first, int count, hipStream_t stream) { return bd_launch_walk(p, first, count, stream); }

}  // namespace clh
