// seed_link.hip -- K7: the chains of one (read, strand) segment linked into paths whose links are colinear, introns or back-splices.
// Definitions: seed_device.h (lk_before, lk_link) and DESIGN.md section 4 (K7); the plain statement is tests/link_check.py.
//
// seed_link_kernel: one wave per segment, lane l holds chain l of at most 64 in registers; nothing goes through LDS or back through
// global memory.  Rank: every lane counts the keys below its own, the other lanes' keys read with cross-lane reads.  The DP visits the
// ranks in order: the owner's fields are broadcast, every lane of lower rank forms its candidate F + lk_link(), and one butterfly on
// (64 value + rank) picks the winner, so that a tie goes to the greatest rank.  Only values above 0 compete, so the packed word is
// positive; F itself may be negative (a chain's score may be) and is multiplied, never shifted.  F, pred and kind stay with the owner.
// The extraction is the same butterfly on (64 F + 63 - rank) over the lanes in no path; the walk reads pred across lanes under a
// wave-uniform mask of used chains, checks every index against [0, n) before it follows it and counts its steps against n.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "seed_device.h"

namespace clh {

static constexpr int kLkWaves = 4;                      // segments of one workgroup: the waves share nothing

__device__ __forceinline__ int64_t lk_wave_max(int64_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const int64_t o = __shfl_xor(v, d);
        v = o > v ? o : v;
    }
    return v;
}

// the lane among the first n whose rank is r, or -1: wave-uniform
__device__ __forceinline__ int lk_lane_of(bool live, int rank, int r)
{
    const unsigned long long b = __ballot(live && rank == r);
    return b ? __ffsll(b) - 1 : -1;
}

__global__ void __launch_bounds__(64 * kLkWaves) seed_link_kernel(LkLaunch L)
{
    const int lane = threadIdx.x & 63;
    const int64_t s = (int64_t)blockIdx.x * kLkWaves + (threadIdx.x >> 6);
    if (s >= L.nseg) return;
    int64_t* hdr = L.lseg + s * kLkSeg;
    const int64_t n64 = L.seg[s * kChSeg];
    if (n64 <= 0 || n64 > L.max_chains || n64 > 64) {    // an empty segment writes its header and leaves; a count out of range is a status
        if (lane == 0) { hdr[0] = 0; hdr[1] = 0; hdr[2] = 0; hdr[3] = n64 == 0 ? 0 : 2; }
        return;
    }
    const int n = (int)n64;
    const bool live = lane < n;
    LkChain me = {0, 0, 0, 0, 0, 0};
    if (live) {
        const int64_t* row = L.rows + (s * L.max_chains + lane) * kChRow;
        me.g = row[2]; me.score = row[3]; me.x0 = row[5]; me.y0 = row[6]; me.x1 = row[7]; me.y1 = row[8];
    }
    int rank = 0;
    for (int m = 0; m < n; ++m) {
        LkChain o = me;
        o.y0 = __shfl(me.y0, m); o.y1 = __shfl(me.y1, m); o.x0 = __shfl(me.x0, m);
        rank += lk_before(o, m, me, lane) ? 1 : 0;
    }
    int64_t F = me.score;
    int pred = -1, kind = 0, status = 0;
    for (int r = 0; r < n && status == 0; ++r) {
        const int o = lk_lane_of(live, rank, r);
        if (o < 0) { status = 3; break; }
        LkChain t;
        t.g = __shfl(me.g, o); t.score = 0; t.x0 = __shfl(me.x0, o); t.x1 = __shfl(me.x1, o); t.y0 = __shfl(me.y0, o); t.y1 = __shfl(me.y1, o);
        int kd = 0;
        int64_t cand = kLkNone;
        if (live && rank < r) {
            const int64_t term = lk_link(me, t, L.p, L.k, &kd);
            if (term != kLkNone && F + term > 0) cand = (F + term) * 64 + rank;
        }
        const int64_t best = lk_wave_max(cand);
        if (best == kLkNone) continue;
        const int j = lk_lane_of(live, rank, (int)(best & 63));
        if (j < 0) { status = 3; break; }
        const int jk = __shfl(kd, j);
        if (lane == o) { F = me.score + best / 64; pred = j; kind = jk; }
    }
    unsigned long long used = 0;
    int paths = 0, path = -1, step = 0, pos = 0;
    int64_t pscore = 0;
    while (status == 0 && paths < n) {
        const int64_t cand = live && !((used >> lane) & 1) ? F * 64 + (63 - rank) : kLkNone;
        const int64_t best = lk_wave_max(cand);
        if (best == kLkNone) break;
        const int e = lk_lane_of(live, rank, 63 - (int)(best & 63));
        if (e < 0) { status = 3; break; }
        const int64_t Fe = __shfl(F, e);
        int i = e, count = 0;
        while (i >= 0 && !((used >> i) & 1)) {
            if (count >= n) { status = 4; break; }
            used |= (unsigned long long)1 << i;
            if (lane == i) { path = paths; step = count; }
            ++count;
            int pi = __builtin_amdgcn_readfirstlane(__shfl(pred, i));
            if (pi < -1 || pi >= n) { status = 3; pi = -1; }     // never followed outside [0, n)
            i = pi;
        }
        const int64_t Fstop = __shfl(F, i >= 0 ? i : 0);
        if (path == paths) {
            pos = count - 1 - step;
            if (pos == 0) pscore = Fe - (i >= 0 ? Fstop : 0);
        }
        ++paths;
    }
    if (live) {
        int64_t* row = L.lrows + (s * L.max_chains + lane) * kLkRow;
        row[0] = rank; row[1] = F; row[2] = pred; row[3] = kind; row[4] = path; row[5] = pos; row[6] = pos == 0 ? pscore : 0; row[7] = 0;
    }
    if (lane == 0) { hdr[0] = n; hdr[1] = paths; hdr[2] = 0; hdr[3] = status; }
}

hipError_t launch_seed_link(const LkLaunch& l, hipStream_t stream)
{
    if (l.nseg <= 0) return hipSuccess;
    hipLaunchKernelGGL(seed_link_kernel, dim3((unsigned)((l.nseg + kLkWaves - 1) / kLkWaves)), dim3(64 * kLkWaves), 0, stream, l);
    return hipGetLastError();
}

}  // namespace clh
