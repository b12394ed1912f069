// edit_align.hip -- K4m / K4t: edlib.align (modes NW, SHW, HW; tasks distance, locations, path) on many pairs (gfx950).
//
// The block scheme is K4's (edit_distance.hip): Myers/Hyyro bit-vector blocks of 64 pattern rows, one lane per block,
// the blocks of a pair in adjacent lanes handing the text symbol and the horizontal delta on with one DPP wave_shr,
// match vectors from the bit planes of the block's pattern symbols, patterns above 4096 symbols swept in passes of 64
// blocks through a per-column byte array.  What differs:
//   * the query is always the pattern (SHW and HW are not symmetric);
//   * the delta entering block 0 is +1 for NW and SHW (row 0 is j), 0 for HW (row 0 is 0);
//   * K4m (EA_SCORE): the last block's lane follows the last-row score in every column and keeps the running minimum and
//     the columns that reach it as a compacted list per pair (reset when the minimum drops, so it ends as exactly the
//     optimal columns).  HW starts the list with column -1 (score m);
//   * reverse pass (EA_REVERSE): SHW of the reversed query against a reversed view of target[0..end], one task per end
//     column, built on the device from K4m's output (launch_edit_align_build_rev); it keeps the last optimal column p,
//     and start = end - p;
//   * K4t (EA_STORE): NW of the query against target[start..end] of the first location storing, per block and column,
//     Pv, Mv and the block's bottom score (20 bytes); edit_align_traceback_kernel walks them back, one lane per pair.
// additionalEqualities: the match vector of a text symbol is OR-ed with those of its partners.
// tools/edit_align_model.py is the same recurrence in Python; tests/edlib_check.py derives every field from the full DP.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "clh_device.h"

namespace clh {

template <int P, bool EQ, int KIND>
__global__ void __launch_bounds__(64) edit_align_kernel(const EaParams prm, const EaTask* __restrict__ tasks, int ntasks, int G)
{
    const int lane = threadIdx.x & 63;
    const int per = 64 / G;
    const int g = lane / G, bl = lane & (G - 1);
    const int tix = blockIdx.x * per + g;
    EaTask task;
    task.pat_off = 0; task.txt_off = 0; task.out_off = 0; task.carry_off = -1; task.pat_len = 0; task.txt_len = 0; task.pair = 0; task.hin0 = 1;
    if (tix < ntasks) task = tasks[tix];
    bool has = tix < ntasks && task.pat_len > 0 && task.txt_len > 0;
    const int m = has ? task.pat_len : 0, n = has ? task.txt_len : 0;
    const int B = (m + 63) >> 6;
    const uint8_t* txt = prm.sym + task.txt_off;
    const int npass = G == 64 ? (B + 63) >> 6 : 1;
    const size_t cstride = (((size_t)n + 63) & ~(size_t)63) + 64;
    int8_t* cbuf[2] = {nullptr, nullptr};
    if (npass > 1) {    // G == 64: one pair per wave, so this is wave-uniform
        if (task.carry_off < 0 || task.carry_off + (int64_t)(2 * cstride) > prm.carry_cap) has = false;
        else { cbuf[0] = prm.carry + task.carry_off; cbuf[1] = cbuf[0] + cstride; }
    }
    const int hin0 = task.hin0;
    // K4m / reverse pass state (meaningful in the last block's lane)
    int best = 0x7fffffff, nb = 0, lastp = -1;
    const int64_t ecap = KIND == EA_SCORE ? (int64_t)n + 1 : 0;   // end slots of this pair
    int32_t* ends = prm.ends + (KIND == EA_SCORE ? task.out_off : 0);
    const bool ends_ok = KIND != EA_SCORE || (task.out_off >= 0 && task.out_off + ecap <= prm.ends_cap);
    // K4t storage of this pair: Pv[B][n], Mv[B][n], S[B][n]
    const bool ws_ok = KIND != EA_STORE || (task.out_off >= 0 && (task.out_off & 7) == 0 &&
                                            task.out_off + (int64_t)20 * B * n <= prm.ws_cap);
    uint64_t* wPv = KIND == EA_STORE ? (uint64_t*)(prm.ws + task.out_off) : nullptr;
    uint64_t* wMv = wPv ? wPv + (size_t)B * n : nullptr;
    int32_t* wS = wPv ? (int32_t*)(wMv + (size_t)B * n) : nullptr;
    if (!ends_ok || !ws_ok) has = false;

    int steps_w = has ? n + (B < 64 ? B : 64) - 1 : 0;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_xor(steps_w, d); steps_w = o > steps_w ? o : steps_w; }
    const int steps = steps_w;

    for (int pass = 0; pass < npass; ++pass) {
        const int blk = pass * 64 + bl;
        const bool active = has && blk < B && bl < G;
        const uint8_t* pat = prm.sym + task.pat_off + 64 * (size_t)blk;
        uint64_t pl[P], vm = 0;
#pragma unroll
        for (int q = 0; q < P; ++q) pl[q] = 0;
        int rows = 0;
        if (active) {
            rows = m - 64 * blk < 64 ? m - 64 * blk : 64;
            for (int k = 0; k < rows; ++k) {
                const uint64_t c = pat[k];
#pragma unroll
                for (int q = 0; q < P; ++q) pl[q] |= ((c >> q) & 1) << k;
            }
            vm = rows == 64 ? ~0ull : ((1ull << rows) - 1);
        }
        uint64_t Pv = ~0ull, Mv = 0;
        const bool is_last = active && blk == B - 1;
        const int lb = rows > 0 ? rows - 1 : 0;
        int bscore = 64 * blk + rows;                    // the block's bottom row in column -1 (row i holds i there)
        if (KIND == EA_SCORE && is_last && hin0 == 0) { best = m; ends[0] = -1; nb = 1; }   // HW: the query before the target
        const int8_t* cin = pass > 0 ? cbuf[(pass - 1) & 1] : nullptr;
        int8_t* cout = pass + 1 < npass ? cbuf[pass & 1] : nullptr;

        uint4 cur = make_uint4(0, 0, 0, 0), nxt = make_uint4(0, 0, 0, 0), ccur = make_uint4(0, 0, 0, 0), cnxt = make_uint4(0, 0, 0, 0);
        const bool feeder = has && bl == 0;
        if (feeder) { __builtin_memcpy(&cur, txt, 16); if (cin) __builtin_memcpy(&ccur, cin, 16); }   // buffers are padded
        int carry = 0;
        for (int t = 0; t < steps; ++t) {
            if ((t & 15) == 0) {
                if (t) { cur = nxt; ccur = cnxt; }
                if (feeder && t + 16 < n) { __builtin_memcpy(&nxt, txt + t + 16, 16); if (cin) __builtin_memcpy(&cnxt, cin + t + 16, 16); }
            }
            const int prev = __builtin_amdgcn_update_dpp(0, carry, 0x138, 0xf, 0xf, true);     // wave_shr:1, lane 0 reads 0
            int c, hin;
            if (bl == 0) {
                const int k = (t >> 2) & 3;
                const uint32_t w = k == 0 ? cur.x : (k == 1 ? cur.y : (k == 2 ? cur.z : cur.w));
                c = (int)((w >> ((t & 3) * 8)) & 0xffu);
                hin = hin0;
                if (cin) {
                    const uint32_t cw = k == 0 ? ccur.x : (k == 1 ? ccur.y : (k == 2 ? ccur.z : ccur.w));
                    hin = (int)(int8_t)((cw >> ((t & 3) * 8)) & 0xffu);
                }
            } else {
                c = prev & 0xff;
                hin = (prev >> 8) - 1;
            }
            const int col = t - bl;
            int hout = 0;
            if (active && col >= 0 && col < n) {
                uint64_t Eq = vm;
#pragma unroll
                for (int q = 0; q < P; ++q) Eq &= ~(pl[q] ^ (((c >> q) & 1) ? ~0ull : 0ull));
                if (EQ) {
                    for (int e = prm.eq_off[c]; e < prm.eq_off[c + 1]; ++e) {
                        const int d = prm.eq_list[e];
                        uint64_t Ed = vm;
#pragma unroll
                        for (int q = 0; q < P; ++q) Ed &= ~(pl[q] ^ (((d >> q) & 1) ? ~0ull : 0ull));
                        Eq |= Ed;
                    }
                }
                const uint64_t Xv = Eq | Mv;
                if (hin < 0) Eq |= 1ull;
                const uint64_t Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
                uint64_t Ph = Mv | ~(Xh | Pv);
                uint64_t Mh = Pv & Xh;
                bscore += (int)((Ph >> lb) & 1ull) - (int)((Mh >> lb) & 1ull);
                hout = (int)(Ph >> 63) - (int)(Mh >> 63);
                Ph <<= 1; Mh <<= 1;
                if (hin < 0) Mh |= 1ull; else if (hin > 0) Ph |= 1ull;
                Pv = Mh | ~(Xv | Ph);
                Mv = Ph & Xv;
                if (cout && bl == 63) cout[col] = (int8_t)hout;
                if (KIND == EA_SCORE && is_last && prm.mode != 0) {
                    if (bscore < best) { best = bscore; ends[0] = col; nb = 1; }
                    else if (bscore == best && nb < ecap) { ends[nb] = col; ++nb; }
                }
                if (KIND == EA_REVERSE && is_last && bscore <= best) { best = bscore; lastp = col; }
                if (KIND == EA_STORE) {
                    const size_t x = (size_t)blk * n + col;
                    wPv[x] = Pv; wMv[x] = Mv; wS[x] = bscore;
                }
            }
            carry = c | ((hout + 1) << 8);
        }
        if (is_last) {
            if (KIND == EA_SCORE) {
                if (prm.mode == 0) { best = bscore; ends[0] = n - 1; nb = 1; }
                prm.best[task.pair] = best;
                prm.cnt[task.pair] = nb;
            }
            if (KIND == EA_REVERSE && task.out_off >= 0 && task.out_off < prm.rev_cap) prm.rev_out[task.out_off] = lastp;
        }
        if (pass + 1 < npass) { __syncthreads(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent"); }
    }
}

// one thread per reverse-pass slot: slot i of pair p handles p's i-th optimal end column (none past the count, none for
// column -1, none when the best is above k)
__global__ void edit_align_build_rev_kernel(const EaParams prm, const EaPair* __restrict__ pairs, const int32_t* __restrict__ slot_pair,
                                            int64_t nslots, EaTask* __restrict__ tasks)
{
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nslots) return;
    const EaPair pr = pairs[slot_pair[s]];
    const int64_t i = s - pr.slot_base;
    EaTask t;
    t.pat_off = pr.rq_off; t.txt_off = pr.rt_off; t.out_off = pr.locbase + i; t.carry_off = -1;
    t.pat_len = 0; t.txt_len = 0; t.pair = slot_pair[s]; t.hin0 = 1;
    const int best = prm.best[t.pair], cnt = prm.cnt[t.pair];
    if (i >= 0 && i < cnt && i <= pr.n && (prm.k < 0 || best <= prm.k) && pr.locbase + i < prm.ends_cap) {
        const int end = prm.ends[pr.locbase + i];
        if (end >= 0 && end < pr.n) {
            // reversed target[0..end] starts at column n - 1 - end of the reversed target; an optimal alignment ending at
            // `end` spans at most m + best columns, so m + best + 1 bound the pass
            const int64_t P = (int64_t)end + 1 < (int64_t)pr.m + best + 1 ? (int64_t)end + 1 : (int64_t)pr.m + best + 1;
            t.txt_off = pr.rt_off + (pr.n - 1 - end);
            t.pat_len = pr.m; t.txt_len = (int32_t)P;
            if (pr.rev_carry_stride > 0) t.carry_off = ((s - pr.rev_s0) % pr.rev_chunk) * pr.rev_carry_stride;
        }
    }
    tasks[s] = t;
}

// one thread per K4t task: target[start..end] of the pair's first location (start from the reverse pass for HW)
__global__ void edit_align_build_path_kernel(const EaParams prm, const EaPair* __restrict__ pairs, const EaPath* __restrict__ paths, int n,
                                             EaTask* __restrict__ tasks)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n) return;
    const EaPath ph = paths[x];
    const EaPair pr = pairs[ph.pair];
    EaTask t;
    t.pat_off = pr.q_off; t.txt_off = pr.t_off; t.out_off = ph.ws_off; t.carry_off = ph.carry_off;
    t.pat_len = pr.m; t.txt_len = -1; t.pair = ph.pair; t.hin0 = 1;
    const int best = prm.best[ph.pair], cnt = prm.cnt[ph.pair];
    if (cnt >= 1 && (prm.k < 0 || best <= prm.k) && pr.locbase < prm.ends_cap) {
        const int end = prm.ends[pr.locbase];
        int start = 0;
        if (prm.mode == 2 && end >= 0) { const int p = prm.rev_out[pr.locbase]; start = p >= 0 ? end - p : -1; }
        const int L = end - start + 1;
        if (start >= 0 && end < pr.n && L >= 0 && L <= ph.lmax) { t.txt_off = pr.t_off + start; t.txt_len = L; }
    }
    tasks[x] = t;
}

__device__ __forceinline__ int ea_H(const uint64_t* Pv, const uint64_t* Mv, const int32_t* S, int L, int i, int j)
{
    if (i == 0) return j;
    if (j == 0) return i;
    const int b = (i - 1) >> 6, r = (i - 1) & 63;
    const uint64_t mask = (2ull << r) - 1;      // rows 0..r of the block (r = 63: all)
    const size_t x = (size_t)b * L + (j - 1);
    const int base = b == 0 ? j : S[x - (size_t)L];
    return base + __popcll(Pv[x] & mask) - __popcll(Mv[x] & mask);
}

// one lane per K4t task: walk back from (m, L) by the rule I, then D, then the diagonal; BAM ops (= 7, X 8, I 1, D 2)
__global__ void edit_align_traceback_kernel(const EaParams prm, const EaPath* __restrict__ paths, const EaTask* __restrict__ tasks, int n,
                                            uint32_t* __restrict__ cigar, int32_t* __restrict__ cig_len)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n) return;
    const EaPath ph = paths[x];
    const EaTask t = tasks[x];
    if (t.txt_len < 0) { cig_len[ph.pair] = -2; return; }           // no path (best above k, or no location)
    const int m = t.pat_len, L = t.txt_len, B = (m + 63) >> 6;
    if (L > 0 && (t.out_off < 0 || t.out_off + (int64_t)20 * B * L > prm.ws_cap)) { cig_len[ph.pair] = -3; return; }
    const uint64_t* Pv = (const uint64_t*)(prm.ws + (L > 0 ? t.out_off : 0));
    const uint64_t* Mv = Pv + (size_t)B * L;
    const int32_t* S = (const int32_t*)(Mv + (size_t)B * L);
    const uint8_t* q = prm.sym + t.pat_off;
    const uint8_t* s = prm.sym + t.txt_off;
    uint32_t* out = cigar + ph.cig_off;
    int i = m, j = L, nops = 0, op = -1, run = 0;
    bool bad = false;
    for (int step = 0; (i > 0 || j > 0) && step <= m + L; ++step) {
        const int h = ea_H(Pv, Mv, S, L, i, j);
        int o;
        if (i > 0 && ea_H(Pv, Mv, S, L, i - 1, j) + 1 == h) { o = 1; --i; }
        else if (j > 0 && ea_H(Pv, Mv, S, L, i, j - 1) + 1 == h) { o = 2; --j; }
        else if (i > 0 && j > 0) {
            const int a = q[i - 1], b = s[j - 1];
            o = (a == b || ((prm.eqm[a * 8 + (b >> 5)] >> (b & 31)) & 1u)) ? 7 : 8;
            --i; --j;
        } else { bad = true; break; }
        if (o == op) ++run;
        else {
            if (run) { if (nops >= ph.cig_cap) { bad = true; break; } out[nops++] = ((uint32_t)run << 4) | (uint32_t)op; }
            op = o; run = 1;
        }
    }
    if (!bad && run) { if (nops >= ph.cig_cap) bad = true; else out[nops++] = ((uint32_t)run << 4) | (uint32_t)op; }
    if (bad || i > 0 || j > 0) { cig_len[ph.pair] = -3; return; }
    for (int a = 0, b = nops - 1; a < b; ++a, --b) { const uint32_t w = out[a]; out[a] = out[b]; out[b] = w; }
    cig_len[ph.pair] = nops;
}

template <int KIND>
static void ea_launch(const EaParams& p, const EaTask* tasks, int ntasks, int G, int planes, bool eq, hipStream_t st)
{
    const dim3 grid((ntasks + 64 / G - 1) / (64 / G)), block(64);
    if (planes <= 3) {
        if (eq) hipLaunchKernelGGL((edit_align_kernel<3, true, KIND>), grid, block, 0, st, p, tasks, ntasks, G);
        else hipLaunchKernelGGL((edit_align_kernel<3, false, KIND>), grid, block, 0, st, p, tasks, ntasks, G);
    } else {
        if (eq) hipLaunchKernelGGL((edit_align_kernel<8, true, KIND>), grid, block, 0, st, p, tasks, ntasks, G);
        else hipLaunchKernelGGL((edit_align_kernel<8, false, KIND>), grid, block, 0, st, p, tasks, ntasks, G);
    }
}

hipError_t launch_edit_align(const EaParams& p, int kind, const EaTask* tasks, int ntasks, int G, int planes, bool eq, hipStream_t stream)
{
    if (ntasks <= 0) return hipSuccess;
    if (kind == EA_SCORE) ea_launch<EA_SCORE>(p, tasks, ntasks, G, planes, eq, stream);
    else if (kind == EA_REVERSE) ea_launch<EA_REVERSE>(p, tasks, ntasks, G, planes, eq, stream);
    else ea_launch<EA_STORE>(p, tasks, ntasks, G, planes, eq, stream);
    return hipGetLastError();
}

hipError_t launch_edit_align_build_rev(const EaParams& p, const EaPair* pairs, const int32_t* slot_pair, int64_t nslots, EaTask* tasks, hipStream_t stream)
{
    if (nslots <= 0) return hipSuccess;
    hipLaunchKernelGGL(edit_align_build_rev_kernel, dim3((unsigned)((nslots + 255) / 256)), dim3(256), 0, stream, p, pairs, slot_pair, nslots, tasks);
    return hipGetLastError();
}

hipError_t launch_edit_align_build_path(const EaParams& p, const EaPair* pairs, const EaPath* paths, int n, EaTask* tasks, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(edit_align_build_path_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, p, pairs, paths, n, tasks);
    return hipGetLastError();
}

hipError_t launch_edit_align_traceback(const EaParams& p, const EaPath* paths, const EaTask* tasks, int n, uint32_t* cigar, int32_t* cig_len, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(edit_align_traceback_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, p, paths, tasks, n, cigar, cig_len);
    return hipGetLastError();
}

}  // namespace clh
