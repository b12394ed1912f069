// ssw_rowscan.h -- what the two row-scan kernels share: K1s (ssw_scan.hip, short reads, 8-bit scores) and K1w (ssw_scan_wide.hip, reads
// up to 4096 bases, both regimes).  Device code (DPP and readlane) but for the last lines: with_geq, the host helper of the launchers.
//
// The matrix is walked row by row: the LANES own reference columns, the loop runs over the read's rows.
//   * a wave is 128 virtual lanes (the 16-bit halves of every VGPR); virtual lane v owns CPR adjacent columns of a chunk
//     of 128*CPR columns (CPR = 2, 4 or 8 by what is left of the window): register t, low halves = columns
//     2*CPR*lane + t, high halves = columns 2*CPR*lane + CPR + t -- the left neighbour of a cell is the same half of the
//     previous register;
//   * one row step (rs_row, rs_lane_carry): diagonal + substitution score (profile of the chunk's columns in LDS, indexed by the
//     row's base: rs_profile_fill, rs_profile_row), the gap from the row above (F; registers), then the gap along the row (E) as a
//     prefix maximum: a dependent chain inside the CPR columns of a virtual lane, one wave-wide scan (6 DPP max) of the per-lane
//     "E leaving the lane" in the frame where a gap extension costs nothing, and the incoming E applied to the lane's columns;
//   * chunks follow each other left to right; the last column of a chunk (H and the E leaving it, per row: rs_handover_out) is
//     handed to the next chunk through two arrays of one short per row, two copies of each by the parity of the chunk (RsHand).
// No fill or drain, no per-cell hand-down: 9 packed operations per cell pair (gap_open == gap_extend) or 13, plus ~40 per
// row step, against ~26 per 128 cells in the anti-diagonal form.
// Below the chunk: the runs of candidate blocks behind the prefilter (rs_pick_count, rs_for_each_run, the static slices), the best of
// an alignment's slices (rs_best_of), the next index of a persistent workgroup (rs_next).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "clh_device.h"
#include "clh_device_ops.h"

namespace clh {
namespace {

static constexpr int RS_CPR_MAX = 8;
static constexpr int RS_PROF_WORDS = 6 * RS_CPR_MAX * 64;      // uint32 per wave: [query code 0..5][register][lane]
static constexpr int RS_INF = 0x7fffffff;

struct RsIn {             // one pass; ScanIn and WIn add what is theirs
    const int8_t* read;   // first row's base
    int rstep;            // +1 / -1
    int L;                // rows of the read
    int rows;             // rows processed: L, or L padded with wildcard rows (score 0 against everything)
    const int8_t* ref;    // first column's base
    int cstep;            // +1 / -1
    int comp;             // reference bytes are complemented as they are read
    int ncols;
    int terminate;        // column maximum that ends the pass (ssw.c:296, 489); 1 << 30 = never
    uint16_t* colmax;     // per-column maxima in processing order, or nullptr
};
struct RsOut { int max, col, row; };

template <int CPR> struct RsVec { static constexpr int VEC = CPR < 4 ? CPR : 4, NCH = CPR / VEC; };      // registers per LDS read, reads per row

__device__ __forceinline__ int rs_read_code(int byte) { const int c = byte & 7; return c > 5 ? 5 : c; }     // a read base as the profile indexes it

// profile of the chunk's columns: prof[q][c][lane][VEC], entry = scores of the row base q against the lane's two columns of register t.
// mat is [6 reference codes][8 read codes].  TR (K1w's transposed form): a column is a read base and the row letter q the reference's.
template <int CPR, bool TR>
__device__ __forceinline__ void rs_profile_fill(const RsIn& in, const int* mat, uint32_t* prof, const int c0)
{
    constexpr int VEC = RsVec<CPR>::VEC, NCH = RsVec<CPR>::NCH;
    const int lane = threadIdx.x & 63;
    int rlo[CPR], rhi[CPR];
#pragma unroll
    for (int t = 0; t < CPR; ++t) {
        const int jlo = c0 + 2 * CPR * lane + t, jhi = jlo + CPR;
        const int blo = jlo < in.ncols ? (int)in.ref[(int64_t)jlo * in.cstep] : 0, bhi = jhi < in.ncols ? (int)in.ref[(int64_t)jhi * in.cstep] : 0;
        rlo[t] = jlo < in.ncols ? (TR ? rs_read_code(blo) : ref_code(blo, in.comp)) : 5;
        rhi[t] = jhi < in.ncols ? (TR ? rs_read_code(bhi) : ref_code(bhi, in.comp)) : 5;
    }
#pragma unroll
    for (int q = 0; q < 6; ++q)
#pragma unroll
        for (int t = 0; t < CPR; ++t) {
            const int slo = TR ? mat[q * 8 + rlo[t]] : mat[rlo[t] * 8 + q], shi = TR ? mat[q * 8 + rhi[t]] : mat[rhi[t] * 8 + q];
            prof[((q * NCH + t / VEC) * 64 + lane) * VEC + (t % VEC)] = (uint32_t)(slo & 0xffff) | ((uint32_t)shi << 16);
        }
}

// the profile entries of the row base q for this lane's registers
template <int CPR>
__device__ __forceinline__ void rs_profile_row(const uint32_t* prof, const int q, const int lane, uint32_t (&P)[CPR])
{
    constexpr int VEC = RsVec<CPR>::VEC, NCH = RsVec<CPR>::NCH;
    const uint32_t* pp = prof + (q * NCH * 64 + lane) * VEC;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        if constexpr (VEC == 4) { const uint4 v = *(const uint4*)(pp + c * 64 * VEC); P[4 * c] = v.x; P[4 * c + 1] = v.y; P[4 * c + 2] = v.z; P[4 * c + 3] = v.w; }
        else { const uint2 v = *(const uint2*)(pp + c * 64 * VEC); P[0] = v.x; P[1] = v.y; }
    }
}

// One row of the lane's columns before the gap entering the lane is known: R[t] = max(diagonal + score, gap from above, gap along the
// row from the lane's own columns).  Hp: the row above; dsrc: where the diagonal comes from (Hp, or the final values of a boundary row
// in K1w); prev_hb: H[row - 1] of the column before the chunk.  NOF (with no_f set): the gap from the row above stays out (K1w's
// boundary rows; compile-time false everywhere else).  Returns U, the E leaving the virtual lane from its own columns.
template <int CPR, bool GEQ, bool NOF = false>
__device__ __forceinline__ uint32_t rs_row(const uint32_t (&dsrc)[CPR], const int prev_hb, const uint32_t (&Hp)[CPR], uint32_t (&Fst)[GEQ ? 1 : CPR],
                                           const uint32_t (&P)[CPR], const uint32_t gO2, const uint32_t gE2, uint32_t (&R)[CPR], const bool no_f = false)
{
    const uint32_t d0 = hand_down(dsrc[CPR - 1], prev_hb);
    uint32_t e = 0;
#pragma unroll
    for (int t = 0; t < CPR; ++t) {
        const uint32_t tt = pk_adds(t == 0 ? d0 : dsrc[t - 1], P[t]);
        uint32_t Fv;
        if constexpr (GEQ) { Fv = pk_subus(Hp[t], gO2); if constexpr (NOF) Fv = no_f ? 0u : Fv; }
        else { Fv = pk_max(pk_subus(Fst[t], gE2), pk_subus(Hp[t], gO2)); Fst[t] = Fv; }
        const uint32_t X = pk_max(tt, Fv);                      // >= 0: Fv is
        if (t == 0) R[0] = X;
        else if constexpr (GEQ) R[t] = pk_max(X, pk_subus(R[t - 1], gO2));
        else { e = pk_max(pk_subus(e, gE2), pk_subus(R[t - 1], gO2)); R[t] = pk_max(X, e); }
    }
    if constexpr (GEQ) return pk_subus(R[CPR - 1], gO2);
    else return pk_max(pk_subus(e, gE2), pk_subus(R[CPR - 1], gO2));
}

// E entering every virtual lane: prefix maximum of U in the frame where crossing a virtual lane costs nothing (K = CPR * gapE is what
// a gap loses across one, kLo = 2 * lane * K).  eb: the E entering the chunk's first column -- the previous chunk, as virtual lane -1.
struct RsCarry { uint32_t Ein; int inc, fill; };      // Ein: packed, at the lane's first column; inc / fill: for rs_handover_out
__device__ __forceinline__ RsCarry rs_lane_carry(const uint32_t U, const int eb, const int K, const int kLo)
{
    const int Blo = (int)(U & 0xffffu) + kLo, Bhi = (int)(U >> 16) + kLo + K;
    RsCarry c;
    c.inc = wave_prefix_max(Blo > Bhi ? Blo : Bhi);
    c.fill = eb - K;
    int exc = dpp_shr1(c.fill, c.inc);
    exc = exc > c.fill ? exc : c.fill;
    const int einLo = exc - kLo + K;
    const int m2 = exc > Blo ? exc : Blo;
    const int einHi = m2 - kLo;
    c.Ein = ((uint32_t)einLo & 0xffffu) | ((uint32_t)einHi << 16);
    return c;
}

// the chunk's last column in row i of the current group of 64: its H (`last`: the lane's last register) and the E that enters the next
// chunk's first column become lane i of cobH / cobE
__device__ __forceinline__ void rs_handover_out(const uint32_t last, const RsCarry& c, const int K, const int i, int& cobH, int& cobE)
{
    const int outH = (int)((uint32_t)__builtin_amdgcn_readlane((int)last, 63) >> 16);
    int outE = __builtin_amdgcn_readlane(c.inc, 63);
    outE = (outE > c.fill ? outE : c.fill) - 127 * K;
    outE = outE < 0 ? 0 : outE;
    const uint32_t li = lane_is(threadIdx.x & 63, i); cobH = set_lane(cobH, outH, li); cobE = set_lane(cobE, outE, li);
}

// the hand-over arrays of a chunk: [2][stride] shorts each, read at the other parity, written at the chunk's (LDS in K1s, HBM in K1w)
struct RsHand {
    const short *Hin, *Ein; short *Hout, *Eout;
    __device__ __forceinline__ RsHand(short* H, short* E, const int parity, const int stride)
        : Hin(H + (parity ^ 1) * stride), Ein(E + (parity ^ 1) * stride), Hout(H + parity * stride), Eout(E + parity * stride) {}
    __device__ __forceinline__ void load(const bool first, const int row, const int rows, int& hbv, int& ebv) const
    { hbv = 0; ebv = 0; if (!first && row < rows) { hbv = Hin[row]; ebv = Ein[row]; } }
    __device__ __forceinline__ void store(const bool more, const int rb, const int cnt, const int cobH, const int cobE) const
    { const int lane = threadIdx.x & 63; if (more && lane < cnt) { Hout[rb + lane] = (short)cobH; Eout[rb + lane] = (short)cobE; } }
};

// the 6 x 8 matrix [reference code][read code] of a chunk's profile, zero outside the caller's n x n; ends with a barrier
__device__ __forceinline__ void rs_stage_matrix(const int8_t* mat, const int n, int* smat)
{
    const int k = threadIdx.x & 63;
    if (k < 48) { const int b = k >> 3, q = k & 7; smat[k] = (b < n && q < n) ? (int)mat[b * n + q] : 0; }
    __syncthreads();
}

// a persistent workgroup's next index from a counter in HBM (wave-uniform)
__device__ __forceinline__ int rs_next(int* counter)
{
    int idx = 0;
    if ((threadIdx.x & 63) == 0) idx = atomicAdd(counter, 1);
    return __builtin_amdgcn_readfirstlane(idx);
}

// the best of up to 64 candidates, one per lane, in every lane: largest score v, then smallest column c, then smallest k (the earlier
// slice -- the one that owns that column)
__device__ __forceinline__ void rs_best_of(int& v, int& c, int& k)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int v2 = __shfl_xor(v, d), c2 = __shfl_xor(c, d), k2 = __shfl_xor(k, d);
        const bool take = v2 > v || (v2 == v && (c2 < c || (c2 == c && k2 < k)));
        v = take ? v2 : v; c = take ? c2 : c; k = take ? k2 : k;
    }
}
// a result row of a window slice that starts at column `base`, in the window's coordinates
__device__ __forceinline__ void rs_shift_row(SswResult& r, const int base)
{
    if (r.score1 > 0) { r.ref_end1 += base; if (r.ref_begin1 >= 0) r.ref_begin1 += base; }
}

// ---- the slices of a long window, behind the prefilter (ssw_prefilter.hip; tools/prefilter_model.py) --------------------------
// Static slices: `own` columns each, started `overlap` columns early.  A local alignment of an L-base read spans at most
// L * (1 + max_match / gap_extend) columns (every deleted reference base costs at least gap_extend, the read can earn at most
// L * max_match), so a slice that starts that many columns (+ 32: the wildcard rows) before the columns it owns computes exactly the H
// of the whole-window pass there.  WIDE (K1w): a slice owns at least twice its overlap.
struct RsSlices { int overlap, own, nstatic; };
template <bool WIDE>
__device__ __forceinline__ RsSlices rs_static_slices(const SswParams& p, const int R, const int L)
{
    RsSlices s;
    s.overlap = L + (L * p.max_match + p.gapE - 1) / p.gapE + 32;
    s.own = (R + 63) / 64; s.own = s.own < 8192 ? 8192 : s.own;
    if (WIDE) s.own = s.own < 2 * s.overlap ? 2 * s.overlap : s.own;
    s.nstatic = (R + s.own - 1) / s.own;
    return s;
}
template <typename F>
__device__ __forceinline__ void rs_for_each_static(const RsSlices& s, const int R, F f)      // f(index, first owned column, end column), a slice per lane
{
    for (int k = threadIdx.x & 63; k < s.nstatic; k += 64) { const long long b = (long long)k * s.own; f(k, (int)b, (int)(b + s.own > R ? R : b + s.own)); }
}

// Candidate blocks: with a score S0 > 0 that is ATTAINED somewhere in the window, every block whose bound d is at most
// thr = (M L - S0) / c is a candidate -- no other block can hold the maximum or tie it.  An alignment that scores S0 or more deletes
// at most (M L - S0) / gapE window bases: it spans no more than L + that many columns, so the candidate slices start that far (+ 32)
// early (ov_c) -- cells that cannot reach S0 may come out lower, they cannot win.  nrun: runs of candidate blocks (cut at groups of 64);
// cost: the columns they would compute; pruned: the runs are few enough (cap) and cost less than the static slices.
struct RsPick { int thr = 0, ov_c = 0, nrun = 0, pruned = 0; long long cost = 0; };      // (as they stand: no candidates; ov_c is the caller's overlap)
template <typename D>
__device__ __forceinline__ RsPick rs_pick_count(const SswParams& p, const D* d, const int nsub, const int R, const int L, const int S0, const RsSlices& s, const int cap)
{
    const int lane = threadIdx.x & 63;
    const int cc = p.max_match < p.gapE ? p.max_match : p.gapE;
    RsPick k;
    k.thr = (p.max_match * L - S0) / cc;
    const int span_s0 = L + (p.max_match * L - S0) / p.gapE + 32;
    k.ov_c = span_s0 < s.overlap ? span_s0 : s.overlap;
    k.nrun = 0; k.cost = 0;
    for (int g = 0; g < nsub; g += 64) {
        const unsigned long long m = __ballot(g + lane < nsub && (int)d[g + lane] <= k.thr);
        k.nrun += __popcll(m & ~(m << 1));
        k.cost += (long long)__popcll(m) * kPfBlock;
    }
    k.cost += (long long)k.nrun * k.ov_c;
    k.pruned = k.nrun <= cap && k.cost < (long long)R + (long long)s.nstatic * s.overlap;
    return k;
}
// every run, in the lane of its first block: f(rank among the runs, first column, end column, blocks, first block)
template <typename D, typename F>
__device__ __forceinline__ void rs_for_each_run(const D* d, const int nsub, const int thr, const int phase, const int R, F f)
{
    const int lane = threadIdx.x & 63;
    int done = 0;
    for (int g = 0; g < nsub; g += 64) {
        const int k = g + lane;
        const unsigned long long m = __ballot(k < nsub && (int)d[k] <= thr);
        const unsigned long long starts = m & ~(m << 1);
        if ((starts >> lane) & 1ull) {
            const unsigned long long rest = ~(m >> lane);              // bit 0 is clear: this lane's block is a candidate
            const int len = rest ? __builtin_ctzll(rest) : 64 - lane;
            int b0 = k * kPfBlock - phase, b1 = (k + len) * kPfBlock - phase;
            b0 = b0 < 0 ? 0 : b0; b1 = b1 > R ? R : b1;
            f(done + __popcll(starts & ((1ull << lane) - 1ull)), b0, b1, len, k);
        }
        done += __popcll(starts);
    }
}
// the alignment's entries of the queue (their first index, wave-uniform) and its line in the control block's counts ...
__device__ __forceinline__ int rs_pick_reserve(const SswParams& p, const int entries, const int pruned, const int R)
{
    int first = 0;
    if ((threadIdx.x & 63) == 0) {
        first = atomicAdd(&p.pf_ctl->qcount, entries);
        if (pruned) atomicAdd(&p.pf_ctl->n_pruned, 1);
        atomicAdd(&p.pf_ctl->cols_window, (unsigned long long)R);
    }
    return __builtin_amdgcn_readfirstlane(first);
}
// ... and, the entries written, the columns they cover (a sum per lane) and the alignment's PfOut
__device__ __forceinline__ void rs_pick_close(const SswParams& p, unsigned long long cols, const PfOut& o)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) cols += __shfl_xor(cols, d);
    if ((threadIdx.x & 63) == 0) { atomicAdd(&p.pf_ctl->cols_scanned, cols); p.pf_out[blockIdx.x] = o; }
}

// host: f(std::true_type) when gap_open == gap_extend (the GEQ kernels), f(std::false_type) else; f launches and returns its error
template <typename F>
inline hipError_t with_geq(const bool geq, F f) { return geq ? f(std::true_type{}) : f(std::false_type{}); }

}  // namespace
}  // namespace clh
