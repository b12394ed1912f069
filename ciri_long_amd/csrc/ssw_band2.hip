// ssw_band2.hip -- K1gb under two-piece affine gap costs: a gap of k letters costs min(go1 + (k-1) ge1, go2 + (k-1) ge2) (gfx950).
//
// The sibling of ssw_band_kernel (ssw_band.hip), in a file of its own so that the one-piece instantiations compile as they did: the
// same frame (lane l owns the CPL band positions b = d - lo = l CPL + k, position b of row i is the cell (i, i + lo + b)), the same
// classes of 2, 4 and 8 positions per lane, the same modes, end cells, tie rules and minus infinity (kBdNeg).  Per row step and lane:
//     F_p[k] = max(Hprev[k+1] - go_p, F_pprev[k+1] - ge_p)            p = 1, 2 (one wave_shl:1 move per piece and for H)
//     T[k]   = max(Hprev[k] + s, F_1[k], F_2[k])                      H without E
//     X_p[k] = T[k] - go_p + (b + 1) ge_p  where the cell exists, else minus infinity;   V_p = max over k of X_p[k]
//     u_p    = exclusive prefix maximum of V_p over the lanes, seeded with minus infinity: two independent wave_prefix_max chains
//     E_p[k] = u_p - b ge_p,  H[k] = max(T[k], E_1[k], E_2[k]) where the cell exists, else minus infinity,  u_p = max(u_p, X_p[k])
// The scan of piece p does not see the other piece's E through H; under 0 <= ge2 <= ge1 <= go1 <= go2 that changes nothing the walk
// reads (the argument is in ssw_ends2.hip; a band only removes cells).  The host's bound takes the maximum over all four costs.
// STORE: one byte per cell -- bits 0..2 H's source (0 diagonal, 1 E_1, 2 E_2, 3 F_1, 4 F_2; that order is the tie rule), bits 3..6
// "opened here" of E_1, E_2, F_1, F_2 -- CPL bytes per lane and row, only the lanes that own a band position: m ceil(B / CPL) CPL bytes
// per pair.  ssw_band2_walk_kernel walks them back with pr_walk2 (ssw_pairs.h).  tests/twopiece_check.py is the definition.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "clh_device.h"
#include "clh_device_ops.h"
#include "ssw_pairs.h"

namespace clh {

template <int CPL> struct Bd2Word;          // a lane's row of decisions: CPL bytes
template <> struct Bd2Word<2> { typedef uint16_t type; };
template <> struct Bd2Word<4> { typedef uint32_t type; };
template <> struct Bd2Word<8> { typedef uint64_t type; };

__device__ __forceinline__ int bd2_min(int a, int b) { return a < b ? a : b; }

template <int CPL, int MODE, bool STORE>
__global__ void __launch_bounds__(64) ssw_band2_kernel(const Bd2Params prm, int first, int count)
{
    typedef typename Bd2Word<CPL>::type word_t;
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
    const int go1 = prm.go, ge1 = prm.ge, go2 = prm.go2, ge2 = prm.ge2;
    const int8_t* qry = prm.qry + pr.q_off;
    const int8_t* ref = prm.ref + pr.r_off;
    const int L = (B + CPL - 1) / CPL;               // lanes with a band position
    const int64_t rowbytes = (int64_t)L * CPL;
    bool ws_ok = true;
    if (STORE) ws_ok = pr.ws_off >= 0 && (pr.ws_off & 15) == 0 && pr.ws_off + (int64_t)m * rowbytes <= prm.ws_cap;
    uint8_t* wsp = (STORE && ws_ok) ? prm.ws + pr.ws_off + (size_t)lane * CPL : nullptr;

    int rc[CPL], jr[CPL], off1[CPL], poff1[CPL], off2[CPL], poff2[CPL], Hp[CPL], F1p[CPL], F2p[CPL];
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
        const int p = lane * CPL + k, j0 = lo + p;             // the position's column in row 0
        jr[k] = p < B ? j0 + 1 : 0x40000000;                   // its column in the row at hand; a position outside the band never is a cell
        rc[k] = (j0 >= 0 && j0 < n) ? ((int)ref[j0] & 31) : 0; // the letter of column j0 + 1, whatever B: it slides down to the band
        poff1[k] = (int)((uint32_t)p * (uint32_t)ge1);
        off1[k] = (int)((uint32_t)(p + 1) * (uint32_t)ge1 - (uint32_t)go1);
        poff2[k] = (int)((uint32_t)p * (uint32_t)ge2);
        off2[k] = (int)((uint32_t)(p + 1) * (uint32_t)ge2 - (uint32_t)go2);
        const bool cell = p < B && j0 >= 0 && j0 <= n;
        const int h0 = (en_anchored(MODE) && j0 > 0) ? -bd2_min(go1 + (j0 - 1) * ge1, go2 + (j0 - 1) * ge2) : 0;
        Hp[k] = cell ? h0 : kBdNeg;
        F1p[k] = kBdNeg;
        F2p[k] = kBdNeg;
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
            const int hnext = dpp_shl1(kBdNeg, Hp[0]), f1next = dpp_shl1(kBdNeg, F1p[0]), f2next = dpp_shl1(kBdNeg, F2p[0]);
            const int* srow = smat + qc * 32;
            int T[CPL], F1[CPL], F2[CPL], D[CPL], H[CPL], E1[CPL], E2[CPL], X1[CPL], X2[CPL], Hu[CPL];
            bool ok[CPL];
            int v1 = kBdNeg, v2 = kBdNeg;
#pragma unroll
            for (int k = 0; k < CPL; ++k) {
                Hu[k] = k + 1 < CPL ? Hp[k + 1] : hnext;
                const int fu1 = k + 1 < CPL ? F1p[k + 1] : f1next, fu2 = k + 1 < CPL ? F2p[k + 1] : f2next;
                F1[k] = pr_max(Hu[k] - go1, fu1 - ge1);
                F2[k] = pr_max(Hu[k] - go2, fu2 - ge2);
                D[k] = Hp[k] + srow[rc[k]];
                ok[k] = (uint32_t)jr[k] <= (uint32_t)n;
                T[k] = pr_max(pr_max(D[k], F1[k]), F2[k]);
                X1[k] = ok[k] ? T[k] + off1[k] : kBdNeg;
                X2[k] = ok[k] ? T[k] + off2[k] : kBdNeg;
                v1 = pr_max(v1, X1[k]);
                v2 = pr_max(v2, X2[k]);
            }
            const int s1 = wave_prefix_max(v1), s2 = wave_prefix_max(v2);
            int u1 = dpp_shr1(kBdNeg, s1), u2 = dpp_shr1(kBdNeg, s2);
#pragma unroll
            for (int k = 0; k < CPL; ++k) {
                E1[k] = u1 - poff1[k];
                E2[k] = u2 - poff2[k];
                H[k] = ok[k] ? pr_max(T[k], pr_max(E1[k], E2[k])) : kBdNeg;
                u1 = pr_max(u1, X1[k]);
                u2 = pr_max(u2, X2[k]);
            }
            if (STORE) {
                const int nleft = dpp_shr1(kBdNeg, H[CPL - 1]);          // H of position b - 1 of this row
                uint64_t w = 0;
#pragma unroll
                for (int k = 0; k < CPL; ++k) {
                    const int left = k ? H[k - 1] : nleft;
                    const uint32_t src = H[k] == D[k] ? 0u : (H[k] == E1[k] ? 1u : (H[k] == E2[k] ? 2u : (H[k] == F1[k] ? 3u : 4u)));
                    const uint32_t b = src | (E1[k] == left - go1 ? 8u : 0u) | (E2[k] == left - go2 ? 16u : 0u) |
                                       (F1[k] == Hu[k] - go1 ? 32u : 0u) | (F2[k] == Hu[k] - go2 ? 64u : 0u);
                    w |= (uint64_t)b << (8 * k);
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
                Hp[k] = H[k]; F1p[k] = F1[k]; F2p[k] = F2[k];
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

// one lane per pair: pr_walk2 over the bytes the storing form left, row after row, in the band's frame
__global__ void ssw_band2_walk_kernel(const Bd2Params prm, int first, int count)
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
    const int64_t rowbytes = (int64_t)((B + cpl - 1) / cpl) * cpl;
    const int64_t nbytes = (int64_t)m * rowbytes;
    if (pr.ws_off < 0 || pr.ws_off + nbytes > prm.ws_cap || pr.cig_off < 0 || pr.cig_off + pr.cig_cap > prm.cigar_cap) { row[7] = EN_ST_NO_WALK; return; }
    const uint8_t* ws = prm.ws + pr.ws_off;
    pr_walk2(row, prm.mode, m, n, prm.cigar + pr.cig_off, pr.cig_cap, [&](int i, int j) -> int {
        const int b = j - i - pr.lo;
        const int64_t bi = (int64_t)(i - 1) * rowbytes + b;
        if (b < 0 || b >= B || i < 1 || bi < 0 || bi >= nbytes) return -1;
        return (int)ws[bi];
    });
}

template <int CPL>
static void bd2_launch(const Bd2Params& p, bool store, int first, int count, hipStream_t st)
{
    if (p.mode == EN_GLOBAL) {
        if (store) hipLaunchKernelGGL((ssw_band2_kernel<CPL, EN_GLOBAL, true>), dim3(count), dim3(64), 0, st, p, first, count);
        else hipLaunchKernelGGL((ssw_band2_kernel<CPL, EN_GLOBAL, false>), dim3(count), dim3(64), 0, st, p, first, count);
    } else if (p.mode == EN_PREFIX) {
        if (store) hipLaunchKernelGGL((ssw_band2_kernel<CPL, EN_PREFIX, true>), dim3(count), dim3(64), 0, st, p, first, count);
        else hipLaunchKernelGGL((ssw_band2_kernel<CPL, EN_PREFIX, false>), dim3(count), dim3(64), 0, st, p, first, count);
    } else if (p.mode == EN_EXTEND) {
        if (store) hipLaunchKernelGGL((ssw_band2_kernel<CPL, EN_EXTEND, true>), dim3(count), dim3(64), 0, st, p, first, count);
        else hipLaunchKernelGGL((ssw_band2_kernel<CPL, EN_EXTEND, false>), dim3(count), dim3(64), 0, st, p, first, count);
    } else {
        if (store) hipLaunchKernelGGL((ssw_band2_kernel<CPL, EN_SEMIGLOBAL, true>), dim3(count), dim3(64), 0, st, p, first, count);
        else hipLaunchKernelGGL((ssw_band2_kernel<CPL, EN_SEMIGLOBAL, false>), dim3(count), dim3(64), 0, st, p, first, count);
    }
}

hipError_t launch_ssw_band2(const Bd2Params& p, int cls, bool store, int first, int count, hipStream_t stream)
{
    if (count <= 0) return hipSuccess;
    if (p.mode != EN_GLOBAL && p.mode != EN_SEMIGLOBAL && p.mode != EN_PREFIX && p.mode != EN_EXTEND) return hipErrorInvalidValue;
    if (cls == 0) bd2_launch<2>(p, store, first, count, stream);
    else if (cls == 1) bd2_launch<4>(p, store, first, count, stream);
    else if (cls == 2) bd2_launch<8>(p, store, first, count, stream);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_ssw_band2_walk(const Bd2Params& p, int first, int count, hipStream_t stream)
{
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(ssw_band2_walk_kernel, dim3((count + 63) / 64), dim3(64), 0, stream, p, first, count);
    return hipGetLastError();
}

}  // namespace clh
