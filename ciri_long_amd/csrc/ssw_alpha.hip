// ssw_alpha.hip -- K1a: ssw_align for substitution matrices of 6..32 letters (protein alphabets), one wavefront per
// alignment (gfx950).
//
// Reproduces ssw_align (reference: libs/striped_smith_waterman/ssw.c:779-869) for any matrix edge n <= 32: the 8-bit pass,
// the 16-bit pass where the 8-bit one overflows (score_size), the NULL of score_size 0, the masked second best, the
// reverse pass for the begin coordinates; the CIGAR comes from ssw_alpha_traceback_kernel (ssw_traceback.hip; ssw.c:548-735).
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
#include "clh_device.h"
#include "clh_device_ops.h"

namespace clh {
namespace {

constexpr int kBig = 1 << 30;

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
        const int cm = wave_max(act ? vMax : 0);
        if (cm > mx) {      // ssw.c:274-291 / 481-495: the first column that raises the maximum
            mx = cm;
            if (BYTE && mx + bias >= 255) { out.overflow = true; break; }
            out.ref = i;
            // ssw.c:299-308 / 502-511 on this column's H: the first row (stripe layout) that holds the maximum
            int r = kBig;
            if (act)
                for (int j = 0; j < segLen; ++j)
                    if ((int)Hs[j * W + s] == mx) { r = row0 + j; break; }
            r = wave_min(r);
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
    int word = 0;
    if (have_byte) {
        b = alpha_pass<16, true>(Ha, Hb, E, seq, L, smat, n, ref, R, false, gO, gE, bias, 255, colmax, global_state);
        if (b.score == 255) {
            if (!have_word) {       // ssw.c:810-813: NULL
                res.status = CLH_STATUS_OVERFLOW8;
                if (lane == 0) { p.results[task.out_index] = res; if (p.cigar_len) p.cigar_len[task.out_index] = 0; }
                return;
            }
            b = alpha_pass<8, false>(Ha, Hb, E, seq, L, smat, n, ref, R, false, gO, gE, 0, 65535, colmax, global_state);
            word = 1;
        }
    } else {
        b = alpha_pass<8, false>(Ha, Hb, E, seq, L, smat, n, ref, R, false, gO, gE, 0, 65535, colmax, global_state);
        word = 1;
    }
    res.score1 = b.score; res.ref_end1 = b.ref; res.read_end1 = b.read;
    res.status = word ? CLH_STATUS_WORD : 0;
    if (task.mask_len >= 15 && colmax) {
        __syncthreads();
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
        second_best(colmax, R, b.ref, task.mask_len, word, res.score2, res.ref_end2);
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

}  // namespace

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

}  // namespace clh
