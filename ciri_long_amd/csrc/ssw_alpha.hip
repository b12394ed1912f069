// ssw_alpha.hip -- K1a: ssw_align for substitution matrices of 6..32 letters (protein alphabets), one wavefront per
// alignment (gfx950).
//
// Reproduces ssw_align (reference: libs/striped_smith_waterman/ssw.c:779-869) for any matrix edge n <= 32: the 8-bit pass,
// the 16-bit pass where the 8-bit one overflows (score_size), the NULL of score_size 0, the masked second best, the
// reverse pass for the begin coordinates; the CIGAR comes from ssw_alpha_traceback_kernel below (ssw.c:548-735).
//
// The passes are the reference's striped loops themselves (oracle/ssw_oracle.c restates them), lane s of the wave being
// stripe s: W = 16 stripes of the 8-bit pass, 8 of the 16-bit pass, segLen = ceil(readLen / W) positions per stripe, row
// r of the read at position r % segLen of stripe r / segLen.  A stripe's positions are a serial chain inside one lane, so
// the lane does what one SSE element does, and what the reference makes observable is kept as it is: the lazy-F loop of
// the 8-bit pass that does not refresh E, the bounded lazy-F loop of the 16-bit pass (F truncated at stripe boundaries
// when gap_open == gap_extend, ssw.c:468-478), the padding rows past the read that score 0 and enter the column maxima,
// the end row as the first row of the stripe layout that holds the maximum.  No part of it depends on the alphabet; only
// the score lookup does: the n x n matrix and the read's codes sit in LDS, a cell reads mat[ref code][read code].
//
// State per pass: H of the previous and current column and E, one int16 per stripe position (6 bytes per read row), in
// LDS up to 8192 rows; longer reads keep the same three arrays in a per-workgroup slot of global memory (`global` form).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <algorithm>
#include "clh_device.h"

namespace clh {
namespace {

constexpr int kBig = 1 << 30;

__device__ __forceinline__ int wmax(int v)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_xor(v, d); v = o > v ? o : v; }
    return v;
}
__device__ __forceinline__ int wmin(int v)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_xor(v, d); v = o < v ? o : v; }
    return v;
}
__device__ __forceinline__ bool wany(bool b) { return __ballot(b) != 0; }
// _mm_slli_si128 by one element over the W stripes: stripe s takes stripe s-1, stripe 0 takes 0
__device__ __forceinline__ int shift_up(int v, int s) { const int t = __shfl_up(v, 1); return s == 0 ? 0 : t; }

struct PassEnd { int score, ref, read; bool overflow; };

// One striped pass (ssw.c:123-345 with BYTE, ssw.c:371-546 without).  seq: the read's codes in row order; the reference
// runs over columns 0..refLen-1, downwards when `down` (the reverse pass).  colmax (forward pass only) receives the
// column maxima; terminate: the column maximum at which the pass stops (ssw.c:297,500).
template <int W, bool BYTE, typename HPtr, typename SPtr>
__device__ PassEnd alpha_pass(HPtr Ha, HPtr Hb, HPtr E, SPtr seq, int readLen, const int8_t* smat, int n, const int8_t* ref,
                              int refLen, bool down, int gapO, int gapE, int bias, int terminate, uint16_t* colmax, bool global_state)
{
    const int s = threadIdx.x & 63;
    const bool act = s < W;
    const int segLen = (readLen + W - 1) / W;
    const int cells = segLen * W;
    for (int k = s; k < cells; k += 64) { Ha[k] = 0; Hb[k] = 0; E[k] = 0; }
    if (global_state) __threadfence();
    __threadfence_block();
    __syncthreads();
    PassEnd out;
    out.score = 0; out.ref = BYTE ? -1 : 0; out.read = readLen - 1; out.overflow = false;    // ssw.c:143-145, 386-388
    int mx = 0;
    const int row0 = s * segLen;
    HPtr Hs = Ha;      // the column being written (pvHStore)
    HPtr Hl = Hb;      // the previous column (pvHLoad)
    int refreg = 0;
    for (int t = 0; t < refLen; ++t) {
        const int i = down ? refLen - 1 - t : t;
        if ((t & 63) == 0) {      // the next 64 reference codes, one per lane
            const int idx = down ? i - s : i + s;
            refreg = (idx >= 0 && idx < refLen) ? (int)ref[idx] : 0;
        }
        int c = __builtin_amdgcn_readlane(refreg, t & 63);
        c = (c < 0 || c >= n) ? 0 : c;                     // (codes were checked before the pass; keeps the lookup inside the matrix)
        const int8_t* mrow = smat + c * n;
        {   HPtr x = Hs; Hs = Hl; Hl = x; }
        // vH = the previous column's last position, shifted one stripe up (ssw.c:190-192)
        int vH = (act && s > 0) ? (int)Hl[(segLen - 1) * W + s - 1] : 0;
        int vF = 0, vMax = 0;
        if (act) {
            for (int j = 0; j < segLen; ++j) {             // ssw.c:204-238 / 441-465
                const int row = row0 + j;
                const int sc = row < readLen ? (int)mrow[(int)seq[row]] : 0;      // rows past the read score 0 (ssw.c:108,363)
                int h;
                if (BYTE) { h = vH + sc + bias; h = h > 255 ? 255 : h; h -= bias; h = h < 0 ? 0 : h; }
                else { h = vH + sc; h = h > 32767 ? 32767 : h; }
                const int k = j * W + s;
                int e = E[k];
                h = h > e ? h : e;
                h = h > vF ? h : vF;
                vMax = vMax > h ? vMax : h;
                Hs[k] = (short)h;
                int h2 = h - gapO; h2 = h2 > 0 ? h2 : 0;
                e -= gapE; e = e > 0 ? e : 0; e = e > h2 ? e : h2;
                E[k] = (short)e;
                vF -= gapE; vF = vF > 0 ? vF : 0; vF = vF > h2 ? vF : h2;
                vH = Hl[k];
            }
        }
        if (BYTE) {         // lazy-F, ssw.c:240-272: until no F can raise an H; E is not refreshed
            vF = shift_up(vF, s); vF = act ? vF : 0;
            int j = 0;
            for (;;) {
                bool need = false;
                if (act) { int hg = (int)Hs[j * W + s] - gapO; hg = hg > 0 ? hg : 0; need = vF > hg; }
                if (!wany(need)) break;
                if (act) {
                    const int k = j * W + s;
                    int h = Hs[k]; h = h > vF ? h : vF;
                    vMax = vMax > h ? vMax : h;
                    Hs[k] = (short)h;
                    vF -= gapE; vF = vF > 0 ? vF : 0;
                }
                if (++j >= segLen) { j = 0; vF = shift_up(vF, s); vF = act ? vF : 0; }
            }
        } else {            // lazy-F, ssw.c:468-478: at most W rounds, the column maximum is not refreshed
            bool done = false;
            for (int kk = 0; kk < W && !done; ++kk) {
                vF = shift_up(vF, s); vF = act ? vF : 0;
                for (int j = 0; j < segLen; ++j) {
                    bool cont = false;
                    if (act) {
                        const int k = j * W + s;
                        int h = Hs[k]; h = h > vF ? h : vF;
                        Hs[k] = (short)h;
                        int h2 = h - gapO; h2 = h2 > 0 ? h2 : 0;
                        vF -= gapE; vF = vF > 0 ? vF : 0;
                        cont = vF > h2;
                    }
                    if (!wany(cont)) { done = true; break; }
                }
            }
        }
        const int cm = wmax(act ? vMax : 0);
        if (cm > mx) {      // ssw.c:274-291 / 481-495: the first column that raises the maximum
            mx = cm;
            if (BYTE && mx + bias >= 255) { out.overflow = true; break; }
            out.ref = i;
            // ssw.c:299-308 / 502-511 on this column's H: the first row (stripe layout) that holds the maximum
            int r = kBig;
            if (act)
                for (int j = 0; j < segLen; ++j)
                    if ((int)Hs[j * W + s] == mx) { r = row0 + j; break; }
            r = wmin(r);
            out.read = r < readLen - 1 ? r : readLen - 1;
        }
        if (colmax && s == 0) colmax[i] = (uint16_t)cm;
        if (cm == terminate) break;
        // the next column reads this one's last positions from the neighbouring lanes
        if (global_state) __threadfence();
        __syncthreads();
    }
    out.score = (BYTE && out.overflow) ? 255 : mx;
    if (mx == 0) out.read = 0;      // no column raised the maximum: the zeroed Hmax holds 0 in row 0 (ssw.c:299-308)
    __syncthreads();
    return out;
}

// masked second-best column maximum, ssw.c:325-340 (8 bit, resumes at edge + 1) / 528-541 (16 bit, at edge); wave-parallel
__device__ void alpha_second_best(const uint16_t* colmax, int refLen, int end_ref, int maskLen, bool word, int& score2, int& ref_end2)
{
    const int lane = threadIdx.x & 63;
    int e1 = end_ref - maskLen; if (e1 < 0) e1 = 0;
    int e2 = end_ref + maskLen; if (e2 > refLen) e2 = refLen;
    e2 += word ? 0 : 1;
    int bv = 0, bp = kBig;
    for (int i = lane; i < refLen; i += 64)
        if (i < e1 || i >= e2) { const int v = colmax[i]; if (v > bv) { bv = v; bp = i; } }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int v2 = __shfl_xor(bv, d), p2 = __shfl_xor(bp, d);
        const bool take = v2 > bv || (v2 == bv && p2 < bp);
        bv = take ? v2 : bv; bp = take ? p2 : bp;
    }
    score2 = bv;
    ref_end2 = bv > 0 ? bp : 0;
}

// the passes of one alignment, ssw.c:779-849
template <typename HPtr, typename SPtr>
__device__ void alpha_align(const SswParams& p, const int8_t* smat, const SswTask& task, HPtr Ha, HPtr Hb, HPtr E, SPtr seq, bool global_state)
{
    const int lane = threadIdx.x & 63;
    const int n = p.n, L = task.read_len, R = task.ref_len;
    const int8_t* read = p.reads + task.read_off;
    const int8_t* ref = p.refs + task.ref_off;
    SswResult res;
    res.score1 = 0; res.score2 = 0; res.ref_begin1 = -1; res.ref_end1 = -1; res.read_begin1 = -1; res.read_end1 = 0;
    res.ref_end2 = 0; res.status = 0;
    // codes outside the matrix: undefined behaviour in the reference, an argument error here (clh_ssw_fetch names the alignment)
    bool bad = false;
    for (int k = lane; k < L; k += 64) { const int c = read[k]; seq[k] = (int8_t)c; bad = bad || c < 0 || c >= n; }
    for (int k = lane; k < R; k += 64) { const int c = ref[k]; bad = bad || c < 0 || c >= n; }
    if (wany(bad)) {
        res.status = CLH_STATUS_BAD_CODE;
        if (lane == 0) { p.results[task.out_index] = res; if (p.cigar_len) p.cigar_len[task.out_index] = 0; }
        return;
    }
    if (global_state) __threadfence();
    __threadfence_block();
    __syncthreads();
    const bool have_byte = p.score_size == 0 || p.score_size == 2, have_word = p.score_size == 1 || p.score_size == 2;
    const int bias = have_byte ? p.bias : 0;
    const int gO = p.gapO, gE = p.gapE;
    uint16_t* colmax = p.colmax ? p.colmax + task.colmax_off : nullptr;
    PassEnd b;
    bool word = false;
    if (have_byte) {
        b = alpha_pass<16, true>(Ha, Hb, E, seq, L, smat, n, ref, R, false, gO, gE, bias, 255, colmax, global_state);
        if (b.score == 255) {
            if (!have_word) {       // ssw.c:810-813: NULL
                res.status = CLH_STATUS_OVERFLOW8;
                if (lane == 0) { p.results[task.out_index] = res; if (p.cigar_len) p.cigar_len[task.out_index] = 0; }
                return;
            }
            b = alpha_pass<8, false>(Ha, Hb, E, seq, L, smat, n, ref, R, false, gO, gE, 0, 65535, colmax, global_state);
            word = true;
        }
    } else {
        b = alpha_pass<8, false>(Ha, Hb, E, seq, L, smat, n, ref, R, false, gO, gE, 0, 65535, colmax, global_state);
        word = true;
    }
    res.score1 = b.score; res.ref_end1 = b.ref; res.read_end1 = b.read;
    res.status = word ? CLH_STATUS_WORD : 0;
    if (task.mask_len >= 15 && colmax) {
        __syncthreads();
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
        alpha_second_best(colmax, R, b.ref, task.mask_len, word, res.score2, res.ref_end2);
    } else { res.score2 = 0; res.ref_end2 = task.mask_len >= 15 ? 0 : -1; }
    const int flag = p.flag;
    if (!(flag == 0 || (flag == 2 && res.score1 < p.filters))) {        // ssw.c:834-849: the begin coordinates
        const int rl = res.read_end1 + 1;
        __syncthreads();
        for (int k = lane; k < rl; k += 64) seq[k] = read[res.read_end1 - k];
        if (global_state) __threadfence();
        __threadfence_block();
        __syncthreads();
        PassEnd r;
        if (!word) r = alpha_pass<16, true>(Ha, Hb, E, seq, rl, smat, n, ref, res.ref_end1 + 1, true, gO, gE, bias, res.score1 & 0xff, nullptr, global_state);
        else r = alpha_pass<8, false>(Ha, Hb, E, seq, rl, smat, n, ref, res.ref_end1 + 1, true, gO, gE, 0, res.score1, nullptr, global_state);
        res.ref_begin1 = r.ref;
        res.read_begin1 = res.read_end1 - r.read;
    }
    if (lane == 0) p.results[task.out_index] = res;
}

__device__ __forceinline__ void stage_matrix(const int8_t* mat, int n, int8_t* smat)
{
    for (int k = threadIdx.x; k < n * n; k += blockDim.x) smat[k] = mat[k];
    __syncthreads();
}

// LDS form: workgroup b takes task b; H, H', E (int16) and the read's codes in dynamic LDS sized for `lcap` rows
__global__ void __launch_bounds__(64) ssw_alpha_kernel(const SswParams p, const int8_t* __restrict__ mat, int lcap)
{
    extern __shared__ __attribute__((aligned(16))) short al_lds[];
    __shared__ int8_t smat[1024];
    stage_matrix(mat, p.n, smat);
    const int cap16 = (lcap + 15) & ~15;
    short* Ha = al_lds;
    short* Hb = al_lds + cap16;
    short* E = al_lds + 2 * cap16;
    int8_t* seq = (int8_t*)(al_lds + 3 * cap16);
    const SswTask task = p.tasks[blockIdx.x];
    alpha_align(p, smat, task, Ha, Hb, E, seq, false);
}

// global form (reads above the LDS form's rows): persistent workgroups, each with a slot of `slot` bytes in `dirs`
__global__ void __launch_bounds__(64) ssw_alpha_global_kernel(const SswParams p, const int8_t* __restrict__ mat, int ntasks, int lcap,
                                                              long long ws_off, int slot)
{
    __shared__ int8_t smat[1024];
    stage_matrix(mat, p.n, smat);
    const int cap16 = (lcap + 15) & ~15;
    uint8_t* base = p.dirs + ws_off + (size_t)blockIdx.x * (size_t)slot;
    short* Ha = (short*)base;
    short* Hb = Ha + cap16;
    short* E = Ha + 2 * cap16;
    int8_t* seq = (int8_t*)(Ha + 3 * cap16);
    for (int t = blockIdx.x; t < ntasks; t += gridDim.x) {
        const SswTask task = p.tasks[t];
        alpha_align(p, smat, task, Ha, Hb, E, seq, true);
        __threadfence();
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// CIGAR: banded_sw (ssw.c:548-735) by anti-diagonals, the formulation of ssw_traceback.hip (K1b's anti-diagonal form; its
// header lists the reference behaviour kept), with the n x n matrix in LDS.  big = 0: every alignment of the class with a
// small LDS window, what outgrows it is listed; big = 1: the listed ones, window sized for the class's longest read.
// ---------------------------------------------------------------------------------------------------------------------
struct AlPool {
    uint8_t* base;
    unsigned long long* head;
    unsigned long long size;
    int* n_big; int* list_big;
    int task_base;
};

__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
__device__ __forceinline__ int ad_first_row(int a, int w) { int t = a - w; return t >= 0 ? (t + 1) >> 1 : -((-t) >> 1); }
__device__ __forceinline__ int ad_lo(int a, int w, int refLen)
{
    int lo = ad_first_row(a, w);
    if (lo < 0) lo = 0;
    const int t = a - (refLen - 1);
    return lo < t ? t : lo;
}
__device__ __forceinline__ int ad_stride(int w, int readLen, int refLen)
{
    int s = w + 1;
    if (s > readLen) s = readLen;
    return s > refLen ? refLen : s;
}

// need: the status bit that lists an alignment for a big != 0 launch (CLH_STATUS_NEED_BIG; CLH_STATUS_NEED_W32 for the DNA alignments
// the 16-bit forms hand over, whose genome windows may be reverse-complemented)
__device__ __forceinline__ void alpha_traceback(const SswParams& p, const int8_t* smat, const AlPool& pool, const int ws, const int wsp, const int big,
                                const int seq_cap, const int task_index, const int need = CLH_STATUS_NEED_BIG)
{
    // int32 state: past the 16-bit pass's ceiling (score1 = 32767) the reference's int DP keeps counting
    extern __shared__ __attribute__((aligned(16))) int tb_lds[];
    int* const H0 = tb_lds;
    int* const E0 = tb_lds + 3 * ws;
    int* const F0 = tb_lds + 5 * ws;
    int8_t* const sseq = (int8_t*)(tb_lds + 7 * ws);
    __shared__ uint8_t stage[64 * 66];
    __shared__ unsigned long long hist_at[24];
    __shared__ int hist_w[24];
    __shared__ unsigned long long s_at;
    __shared__ int s_max[16];
    const int lane = threadIdx.x;
    const int nt = blockDim.x;
    const SswTask task = p.tasks[task_index];
    SswResult res = p.results[task.out_index];
    res.score1 = __builtin_amdgcn_readfirstlane(res.score1); res.status = __builtin_amdgcn_readfirstlane(res.status);
    res.ref_begin1 = __builtin_amdgcn_readfirstlane(res.ref_begin1); res.ref_end1 = __builtin_amdgcn_readfirstlane(res.ref_end1);
    res.read_begin1 = __builtin_amdgcn_readfirstlane(res.read_begin1); res.read_end1 = __builtin_amdgcn_readfirstlane(res.read_end1);
    uint32_t* cig = p.cigars + task.cigar_off;
    int* cig_len = p.cigar_len + task.out_index;
    if (big) {
        if (!(res.status & need)) return;
        res.status &= ~need;
        __syncthreads();        // every wave has read the row (and found the bit) before it is cleared in memory
        if (lane == 0) p.results[task.out_index].status = res.status;
    }
    const bool no_cigar = (res.status & (CLH_STATUS_OVERFLOW8 | CLH_STATUS_BAD_CODE)) || (7 & p.flag) == 0 ||
                          ((2 & p.flag) != 0 && res.score1 < p.filters) ||
                          ((4 & p.flag) != 0 && (res.ref_end1 - res.ref_begin1 > p.filterd || res.read_end1 - res.read_begin1 > p.filterd));
    if (no_cigar) {
        if (lane == 0) { *cig_len = 0; p.results[task.out_index].status = res.status | CLH_STATUS_NO_CIGAR; }
        return;
    }
    if (res.ref_begin1 < 0) {   // score 0: the reference's 1x1 problem never enters its traceback loop -> 1M
        if (lane == 0) { cig[0] = (1u << 4); *cig_len = 1; }
        return;
    }
    // DNA (need == CLH_STATUS_NEED_W32): reference bytes through ref_code, as the 16-bit forms read them (genome windows: case and N
    // flags, reverse complement); K1a's references are packed codes, forward
    const bool dna = need == CLH_STATUS_NEED_W32;
    const int rdir = task.ref_rc ? -1 : 1, rc = task.ref_rc;
    const int8_t* ref = p.refs + task.ref_off + (int64_t)res.ref_begin1 * rdir;
    const int8_t* read = p.reads + task.read_off + res.read_begin1;
    const int refLen = res.ref_end1 - res.ref_begin1 + 1, readLen = res.read_end1 - res.read_begin1 + 1;
    const int score = res.score1, gO = p.gapO, gE = p.gapE, n = p.n;
    // both sequences in LDS where they fit; the large configuration reads what does not fit from global memory
    const bool staged = readLen + refLen <= seq_cap;
    if (!staged && big != 1) {
        if (lane == 0) {
            *cig_len = 0; p.results[task.out_index].status = res.status | CLH_STATUS_NEED_BIG;
            pool.list_big[atomicAdd(pool.n_big, 1)] = task_index;
        }
        return;
    }
    if (staged) {
        for (int k = lane; k < readLen; k += nt) sseq[k] = read[k];
        for (int k = lane; k < refLen; k += nt) sseq[readLen + k] = dna ? (int8_t)ref_code((int)ref[(int64_t)k * rdir], rc) : ref[k];
    }
    __syncthreads();
    const int8_t* const sread = staged ? sseq : read;
    const int8_t* const sref = staged ? sseq + readLen : ref;
    auto ref_at = [&](int j) -> int { return (staged || !dna) ? (int)sref[j] : ref_code((int)ref[(int64_t)j * rdir], rc); };
    int w = refLen > readLen ? refLen - readLen : readLen - refLen;
    w += 1;
    const int nAD = readLen + refLen - 1;
    int maxv = 0;
    uint8_t* dir = nullptr;
    int status = 0, niter = 0;
    bool covered = false;
    unsigned long long last_at = 0;

    for (;;) {
        const int stride_w = ad_stride(w, readLen, refLen);
        if (covered) {
            if (lane == 0 && niter < 24) { hist_at[niter] = last_at; hist_w[niter] = w; }
            ++niter;
            w *= 2;
            if (!(maxv < score && w < 2 * readLen)) break;
            continue;
        }
        const bool ring = w + 3 <= wsp;
        if (!ring && readLen + 1 > ws) { status = big == 1 ? CLH_STATUS_CIGAR_TRUNC : CLH_STATUS_NEED_BIG; break; }
        const int imask = ring ? wsp - 1 : -1;
        unsigned long long need = ((unsigned long long)nAD * (unsigned long long)stride_w + 63ull) & ~63ull;
        unsigned long long at = 0;
        __syncthreads();
        if (lane == 0) s_at = atomicAdd(pool.head, need);
        __syncthreads();
        at = (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(s_at & 0xffffffffull)) | ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(s_at >> 32)) << 32);
        // the pool ran out: K1a's alignments go round again over the emptied pool (clh_ssw_fetch), the DNA ones report it
        if (at + need > pool.size) { status = dna ? CLH_STATUS_CIGAR_TRUNC : CLH_STATUS_NEED_POOL; break; }
        dir = pool.base + at;
        last_at = at;
        if (lane == 0 && niter < 24) { hist_at[niter] = at; hist_w[niter] = w; }
        ++niter;
        covered = w >= readLen && w >= refLen;
        int itmax = 0;
        for (int a = 0; a < nAD; ++a) {
            const int cur = a % 3, p1 = (a + 2) % 3, p2 = (a + 1) % 3, e0 = a & 1, e1 = e0 ^ 1;
            const int ilo = ad_lo(a, w, refLen);
            int ihi = (a + w) >> 1;
            if (ihi > readLen - 1) ihi = readLen - 1;
            if (ihi > a) ihi = a;
            for (int i0 = ilo; i0 <= ihi; i0 += nt) {
                const int i = i0 + lane;
                if (i <= ihi) {
                    const int j = a - i;
                    const int m = i & imask, mu = (i - 1) & imask;
                    int hu = 0, eu = 0, hl = 0, fl = 0, hd = 0;
                    if (i >= 1) {
                        const bool up_in = j <= i - 1 + w;
                        const bool clobber = (i - 1 <= w) && (refLen - 1 < i + w) && (j == refLen - 1);
                        if (up_in && !clobber) { hu = H0[p1 * ws + mu]; eu = E0[e1 * ws + mu]; }
                        if (j >= 1) hd = H0[p2 * ws + mu];
                    }
                    if (j >= 1 && j - 1 >= i - w) { hl = H0[p1 * ws + m]; fl = F0[e1 * ws + m]; }
                    int t1 = i == 0 ? -gO : hu - gO, t2 = i == 0 ? -gE : eu - gE;
                    const int e = t1 > t2 ? t1 : t2;
                    const int de = t1 > t2 ? 3 : 2;
                    t1 = hl - gO; t2 = fl - gE;
                    const int f = t1 > t2 ? t1 : t2;
                    const int df = t1 > t2 ? 5 : 4;
                    const int e1v = e > 0 ? e : 0, f1v = f > 0 ? f : 0;
                    t1 = e1v > f1v ? e1v : f1v;
                    t2 = hd + smat[ref_at(j) * n + (int)sread[i]];
                    const int h = t1 > t2 ? t1 : t2;
                    const int dh = t1 <= t2 ? 1 : (e1v > f1v ? de : df);
                    itmax = h > itmax ? h : itmax;
                    H0[cur * ws + m] = h; E0[e0 * ws + m] = e; F0[e0 * ws + m] = f;
                    dir[(size_t)a * stride_w + (i - ilo)] = (uint8_t)(dh | (de == 3 ? 8 : 0) | (df == 5 ? 16 : 0));
                }
            }
            lds_barrier();
        }
        itmax = wmax(itmax);
        if ((lane & 63) == 0) s_max[lane >> 6] = itmax;
        __syncthreads();
        for (int k = 0; k < (nt >> 6); ++k) itmax = s_max[k] > itmax ? s_max[k] : itmax;
        itmax = __builtin_amdgcn_readfirstlane(itmax);
        maxv = itmax > maxv ? itmax : maxv;
        w *= 2;
        if (!(maxv < score && w < 2 * readLen)) break;
    }
    if (status) {
        if (lane == 0) {
            *cig_len = 0; p.results[task.out_index].status = res.status | status;
            if (status == CLH_STATUS_NEED_BIG) pool.list_big[atomicAdd(pool.n_big, 1)] = task_index;
        }
        return;
    }
    w /= 2;
    // the walk reads direction bytes other waves stored: the stores must have reached L2 and this CU's L1 must not serve old lines
    // (a workgroup-scope fence does not wait for them: the last anti-diagonals' bytes could still be in flight)
    __threadfence();
    __syncthreads();

    // walk back from the bottom-right corner (ssw.c:636-696); a step outside the final band reads the byte an earlier,
    // narrower iteration left at that index of the reference's flat array (every iteration's bytes are still in the pool)
    int i = readLen - 1, j = refLen - 1, state = 2, run = 0, nops = 0, fail = 0;
    int op = 0, prev_op = 0;
    const int stride = ad_stride(w, readLen, refLen);
    int st_lo = 1 << 30, st_hi = -1, st_base = 0;
    const long long wd_final = 2ll * w + 1;
    while (i > 0) {
        int code = 0;
        if (j >= 0 && j <= i + w && j >= i - w && j < refLen) {
            const int a = i + j;
            const int slot = i - ad_lo(a, w, refLen);
            if (a < st_lo || a > st_hi || slot < st_base || slot >= st_base + 64) {
                st_hi = a; st_lo = a - 63 > 0 ? a - 63 : 0; st_base = slot - 32;
                __syncthreads();
                for (int b = lane; b < 64 * 64; b += nt) {
                    const int aa = st_lo + (b >> 6), t = st_base + (b & 63);
                    stage[b] = (aa <= st_hi && t >= 0 && t < stride) ? dir[(size_t)aa * stride + t] : (uint8_t)0;
                }
                __syncthreads();
            }
            code = stage[(a - st_lo) * 64 + (slot - st_base)];
        } else {
            const long long xi = i - w > 0 ? i - w : 0;
            const long long C = (long long)i * wd_final + ((long long)j - xi);
            code = -1;
            if (C >= 0 && niter <= 24) {
                for (int k = niter - 1; k >= 0; --k) {
                    const long long wk = hist_w[k], wd = 2 * wk + 1;
                    const long long ii = C / wd, pos = C % wd;
                    if (ii >= readLen) continue;
                    const long long xk = ii - wk > 0 ? ii - wk : 0, jj = xk + pos;
                    const long long endk = ii + wk < refLen - 1 ? ii + wk : refLen - 1;
                    if (jj > endk) continue;
                    const int a = (int)(ii + jj);
                    code = pool.base[hist_at[k] + (size_t)a * (size_t)ad_stride((int)wk, readLen, refLen) + (size_t)(ii - ad_lo(a, (int)wk, refLen))];
                    break;
                }
            }
            if (code < 0) { fail = 1; break; }
        }
        const int c = state == 2 ? (code & 7) : (state == 0 ? ((code & 8) ? 3 : 2) : ((code & 16) ? 5 : 4));
        switch (c) {
            case 1: --i; --j; state = 2; op = 0; break;
            case 2: --i; state = 0; op = 1; break;
            case 3: --i; state = 2; op = 1; break;
            case 4: --j; state = 1; op = 2; break;
            case 5: --j; state = 2; op = 2; break;
            default: fail = 1; break;
        }
        if (fail) break;
        if (op == prev_op) ++run;
        else {
            if (nops < task.cigar_cap && lane == 0) cig[nops] = ((uint32_t)run << 4) | (uint32_t)prev_op;
            ++nops; prev_op = op; run = 1;
        }
    }
    if (fail) {
        if (lane == 0) { *cig_len = 0; p.results[task.out_index].status = res.status | CLH_STATUS_TRACE_ERR;
 }
        return;
    }
    if (op == 0) {                                   // ssw.c:697-714
        if (nops < task.cigar_cap && lane == 0) cig[nops] = ((uint32_t)(run + 1) << 4);
        ++nops;
    } else {
        if (nops < task.cigar_cap && lane == 0) cig[nops] = ((uint32_t)run << 4) | (uint32_t)op;
        ++nops;
        if (nops < task.cigar_cap && lane == 0) cig[nops] = (1u << 4);
        ++nops;
    }
    if (nops > task.cigar_cap) {
        if (lane == 0) { *cig_len = 0; p.results[task.out_index].status = res.status | CLH_STATUS_CIGAR_TRUNC; }
        return;
    }
    __threadfence_block();
    __syncthreads();
    for (int k = lane; k < nops / 2; k += nt) {      // reverse in place, ssw.c:716-725
        const uint32_t x = cig[k], y = cig[nops - 1 - k];
        cig[k] = y; cig[nops - 1 - k] = x;
    }
    if (lane == 0) *cig_len = nops;
}

// big != 0: the alignments listed in pool.list_big that carry the status bit `need` (CLH_STATUS_NEED_BIG, or CLH_STATUS_NEED_POOL for a
// round over the emptied pool)
__global__ void __launch_bounds__(1024) ssw_alpha_traceback_kernel(const SswParams p, const int8_t* __restrict__ mat, AlPool pool, int ws, int wsp,
                                                                   int big, int seq_cap, int need)
{
    __shared__ int8_t smat[1024];
    stage_matrix(mat, p.n, smat);
    if (big == 0) { alpha_traceback(p, smat, pool, ws, wsp, big, seq_cap, pool.task_base + (int)blockIdx.x); return; }
    const int nb = __builtin_amdgcn_readfirstlane(*pool.n_big);
    for (int k = (int)blockIdx.x; k < nb; k += (int)gridDim.x) {
        alpha_traceback(p, smat, pool, ws, wsp, big, seq_cap, __builtin_amdgcn_readfirstlane(pool.list_big[k]), need);
        __syncthreads();
    }
}

// The DNA alignments the 16-bit traceback forms marked CLH_STATUS_NEED_W32 among tasks [task_base, task_base + ntasks): the workgroups
// split the range, each scans its part a block at a time (the marked ones are few) and runs the int32 traceback on what it finds.
__global__ void __launch_bounds__(1024) ssw_w32_traceback_kernel(const SswParams p, AlPool pool, int ws, int wsp, int seq_cap, int ntasks)
{
    __shared__ int8_t smat[1024];
    __shared__ int s_n, s_list[1024];
    if ((int)threadIdx.x < p.n * p.n) smat[threadIdx.x] = p.mat[threadIdx.x];
    const int per = (ntasks + (int)gridDim.x - 1) / (int)gridDim.x;
    const int k0 = (int)blockIdx.x * per, k1 = min(ntasks, k0 + per);
    for (int b = k0; b < k1; b += (int)blockDim.x) {
        if (threadIdx.x == 0) s_n = 0;
        __syncthreads();
        const int k = b + (int)threadIdx.x;
        if (k < k1) {
            const SswTask& t = p.tasks[pool.task_base + k];
            if (t.out_index < p.n_real && (p.results[t.out_index].status & CLH_STATUS_NEED_W32)) s_list[atomicAdd(&s_n, 1)] = pool.task_base + k;
        }
        __syncthreads();
        const int nf = __builtin_amdgcn_readfirstlane(s_n);
        for (int q = 0; q < nf; ++q) {
            alpha_traceback(p, smat, pool, ws, wsp, 1, seq_cap, __builtin_amdgcn_readfirstlane(s_list[q]), CLH_STATUS_NEED_W32);
            __syncthreads();
        }
    }
}

}  // namespace

hipError_t launch_traceback_w32(const SswParams& p, int task_base, int ntasks, uint8_t* pool_base, unsigned long long* pool_head,
                                unsigned long long pool_size, hipStream_t stream)
{
    if (ntasks <= 0) return hipSuccess;
    AlPool pool; pool.base = pool_base; pool.head = pool_head; pool.size = pool_size; pool.task_base = task_base;
    pool.n_big = nullptr; pool.list_big = nullptr;           // (a big = 1 pass lists nothing)
    const int ws = 5122;                                      // H/E/F (int32) of 5120 rows, the rest of 146 KiB for the sequences
    int wsp = 1;
    while (wsp * 2 <= ws) wsp *= 2;
    const int seq_cap = 149504 - 7 * ws * (int)sizeof(int);  // (4 KiB less than K1a's large launch: the kernel's list of marked tasks)
    const size_t lds = (size_t)7 * ws * sizeof(int) + (size_t)seq_cap;
    // a few workgroups (each holds a CU's LDS): the marked alignments are rare, and most launches only scan
    const int grid = std::min((ntasks + 255) / 256, 64);
    hipLaunchKernelGGL(ssw_w32_traceback_kernel, dim3(grid), dim3(1024), lds, stream, p, pool, ws, wsp, seq_cap, ntasks);
    return hipGetLastError();
}

size_t alpha_lds_bytes(int lcap) { return (size_t)3 * (size_t)((lcap + 15) & ~15) * sizeof(short) + (size_t)lcap + 16; }

hipError_t launch_ssw_alpha(const SswParams& p, const int8_t* d_mat, int ntasks, int lcap, int nworkgroups, long long ws_off, int ws_slot,
                            hipStream_t stream)
{
    if (ntasks <= 0) return hipSuccess;
    if (lcap <= kAlphaLdsRows) {
        hipLaunchKernelGGL(ssw_alpha_kernel, dim3(ntasks), dim3(64), alpha_lds_bytes(lcap), stream, p, d_mat, lcap);
    } else {
        hipLaunchKernelGGL(ssw_alpha_global_kernel, dim3(nworkgroups), dim3(64), 0, stream, p, d_mat, ntasks, lcap, ws_off, ws_slot);
    }
    return hipGetLastError();
}

// the small-window attempt for every alignment of the class, then the listed ones with a window for rows <= lmax
hipError_t launch_ssw_alpha_traceback(const SswParams& p, const int8_t* d_mat, int task_base, int ntasks, int n_total, int seg, int lmax,
                                      uint8_t* pool_base, unsigned long long* pool_head, unsigned long long pool_size, hipStream_t stream)
{
    if (ntasks <= 0) return hipSuccess;
    AlPool pool; pool.base = pool_base; pool.head = pool_head; pool.size = pool_size; pool.task_base = task_base;
    int *n_small, *list_small;
    tb_lists_of(pool_head, n_total, seg, task_base, &n_small, &pool.n_big, &list_small, &pool.list_big);
    for (int big = 0; big < 2; ++big) {
        // big: H/E/F (int32) of the class's longest read (+2), the rest of 150 KiB for the sequences
        const int ws = big ? std::min(lmax + 2, 5122) : 514;
        int wsp = 1;
        while (wsp * 2 <= ws) wsp *= 2;
        const int seq_cap = big ? 153600 - 7 * ws * (int)sizeof(int) : 6144;
        const size_t lds = (size_t)7 * ws * sizeof(int) + (size_t)seq_cap;
        const int grid = big == 0 ? ntasks : std::min(ntasks, 512);
        hipLaunchKernelGGL(ssw_alpha_traceback_kernel, dim3(grid), dim3(big ? 1024 : 128), lds, stream, p, d_mat, pool, ws, wsp, big, seq_cap,
                           (int)CLH_STATUS_NEED_BIG);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// the large configuration whatever the class (a window sized for 5 120 rows gives every alignment the CIGAR its class's own would);
// one_by_one: a single workgroup, which takes the listed alignments in list order
hipError_t launch_ssw_alpha_traceback_retry(const SswParams& p, const int8_t* d_mat, int* d_list, int nlist, bool one_by_one, uint8_t* pool_base,
                                            unsigned long long* pool_head, unsigned long long pool_size, hipStream_t stream)
{
    if (nlist <= 0) return hipSuccess;
    AlPool pool; pool.base = pool_base; pool.head = pool_head; pool.size = pool_size; pool.task_base = 0;
    pool.n_big = d_list; pool.list_big = d_list + 1;
    const int ws = 5122, wsp = 4096;
    const int seq_cap = 153600 - 7 * ws * (int)sizeof(int);
    const size_t lds = (size_t)7 * ws * sizeof(int) + (size_t)seq_cap;
    hipError_t e = hipMemsetAsync(pool_head, 0, sizeof(unsigned long long), stream);      // the bump pointer only
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ssw_alpha_traceback_kernel, dim3(one_by_one ? 1 : std::min(nlist, 512)), dim3(1024), lds, stream, p, d_mat, pool, ws, wsp, 1, seq_cap,
                       (int)CLH_STATUS_NEED_POOL);
    return hipGetLastError();
}

}  // namespace clh
