// seed.hip -- K7: minimizer sketch, seed look-up and colinear chaining on the resident genome (K5), the producer of the loci that
// extend_anchors_genome, align_windows_band and align_windows_spliced take.  Definitions: seed_device.h and DESIGN.md section 4 (K7); the
// plain statement every array is compared with is tests/seed_check.py.  Nothing here has a counterpart in the reference, whose mapper is
// an external package.
//
// Sketch (seed_sketch_kernel, counting and filling form): one wave per work item of kSdItem positions of one sequence (a contig, a read).
// The wave stages the item's letters and the k + w' - 2 on either side that its positions can see into LDS (the only global reads: a byte
// per base and that overlap), rolls f / r over a stretch of them per lane (sd_roll_push: the one packing, sd_roll_key: the one mix) and
// leaves (key << 1 | strand) per position in LDS.  Then lane l decides position round * 64 + l (sd_selected: the per-position rule), and a
// ballot puts the selected ones of the round in position order behind those of the rounds before: no atomics, entries come out sorted by
// (sequence, position).  The counting form leaves one count per item; their scan (seed_sort.hip) gives the filling form its offsets.
//
// Look-up: a thread per read minimizer, two binary searches in the sorted keys (a dependent chain of log2(entries) loads); a scan of the
// counts; a thread per minimizer writes its anchors as two sort words, (read << 1 | minus) and (x << 24 | y); two stable radix sorts
// (seed_sort.hip) put them in (read, minus, x, y) order.
//
// Chain (seed_chain_kernel): one wave per (read, strand) segment, anchors in sequence, the 64 lanes on the 64 candidate predecessors,
// whose x, y, f and contig sit in an LDS ring; one butterfly per anchor on (64 value + 63 - distance), so that a tie goes to the nearest.
// The extraction walks p() under the segment's anchor count; every index is checked against the segment before it is followed.  f, p and
// the used marks are stored by every lane alike, so a lane reads back only what it wrote itself.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "seed_device.h"

namespace clh {

template <bool FILL>
__global__ void __launch_bounds__(64 * kSdItemsPerBlock) seed_sketch_kernel(SdSketch s, int32_t* __restrict__ item_count, const int64_t* __restrict__ item_off,
                                                                           uint64_t* __restrict__ keys, uint64_t* __restrict__ vals, int32_t* __restrict__ seq_of,
                                                                           int64_t cap)
{
    __shared__ uint64_t s_key[kSdItemsPerBlock][kSdKeysCap];
    __shared__ uint8_t s_let[kSdItemsPerBlock][(kSdLettersCap + 15) & ~15];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t item = (int64_t)blockIdx.x * kSdItemsPerBlock + wave;
    uint64_t* vkey = s_key[wave];
    uint8_t* let = s_let[wave];
    const int k = s.k;
    const uint64_t m = ((uint64_t)1 << (2 * k)) - 1;
    bool active = item < s.nitems;
    int seq = 0;
    int64_t off = 0, P = 0, p0 = 0, p1 = 0, klo = 0, khi = 0;
    int wp = 1;
    if (active) {
        seq = s.item_seq[item];
        active = seq >= 0 && seq < s.nseq;
    }
    if (active) {
        off = s.off[seq];
        const int64_t len = s.len[seq];
        P = len - k + 1;
        p0 = (item - s.seq_item0[seq]) * kSdItem;
        active = off >= 0 && len >= 0 && off + len <= s.codes_len && p0 >= 0 && p0 < P;
    }
    if (active) {
        wp = (int)(P < s.w ? P : s.w);
        p1 = p0 + kSdItem < P ? p0 + kSdItem : P;
        klo = p0 - (wp - 1) > 0 ? p0 - (wp - 1) : 0;
        khi = p1 + (wp - 1) < P ? p1 + (wp - 1) : P;
    }
    const int nkeys = (int)(khi - klo);                  // <= kSdKeysCap
    if (active) {
        const int nlet = nkeys + k - 1;                  // <= kSdLettersCap; the last letter is off + khi + k - 2 <= off + len - 1
        for (int t = lane; t < nlet; t += 64) let[t] = s.codes[off + klo + t];
    }
    __syncthreads();
    if (active) {
        const int per = (nkeys + 63) / 64;
        const int t0 = lane * per, t1 = t0 + per < nkeys ? t0 + per : nkeys;
        if (t0 < t1) {
            SdRoll roll;
            sd_roll_init(&roll);
            for (int t = t0; t < t0 + k - 1; ++t) sd_roll_push(&roll, let[t], k, m);
            for (int t = t0; t < t1; ++t) {
                sd_roll_push(&roll, let[t + k - 1], k, m);
                vkey[t] = sd_roll_key(roll, k, m);
            }
        }
    }
    __syncthreads();
    if (!active) {
        if (!FILL && item < s.nitems && lane == 0) item_count[item] = 0;
        return;
    }
    int64_t base = FILL ? item_off[item] : 0;
    int total = 0;
    for (int64_t r0 = p0; r0 < p1; r0 += kSdRound) {
        const int64_t p = r0 + lane;
        const bool sel = p < p1 && sd_selected(vkey, klo, khi, p, wp);
        const unsigned long long bal = __ballot(sel);
        if (FILL) {
            const int64_t e = base + __popcll(bal & (((unsigned long long)1 << lane) - 1));
            if (sel && e >= 0 && e < cap) {
                const uint64_t v = vkey[p - klo];
                keys[e] = v >> 1;
                vals[e] = ((uint64_t)(s.global_pos ? off + p : p) << 1) | (v & 1);
                if (seq_of) seq_of[e] = seq;
            }
            base += __popcll(bal);
        } else {
            total += __popcll(bal);
        }
    }
    if (!FILL && lane == 0) item_count[item] = total;
}

hipError_t launch_seed_sketch_count(const SdSketch& s, int32_t* item_count, hipStream_t stream)
{
    if (s.nitems <= 0) return hipSuccess;
    hipLaunchKernelGGL(seed_sketch_kernel<false>, dim3((unsigned)((s.nitems + kSdItemsPerBlock - 1) / kSdItemsPerBlock)), dim3(64 * kSdItemsPerBlock), 0, stream, s,
                       item_count, (const int64_t*)nullptr, (uint64_t*)nullptr, (uint64_t*)nullptr, (int32_t*)nullptr, (int64_t)0);
    return hipGetLastError();
}

hipError_t launch_seed_sketch_fill(const SdSketch& s, const int64_t* item_off, uint64_t* keys, uint64_t* vals, int32_t* seq_of, int64_t cap, hipStream_t stream)
{
    if (s.nitems <= 0 || cap <= 0) return hipSuccess;
    hipLaunchKernelGGL(seed_sketch_kernel<true>, dim3((unsigned)((s.nitems + kSdItemsPerBlock - 1) / kSdItemsPerBlock)), dim3(64 * kSdItemsPerBlock), 0, stream, s,
                       (int32_t*)nullptr, item_off, keys, vals, seq_of, cap);
    return hipGetLastError();
}

__global__ void __launch_bounds__(256) seed_index_stats_kernel(const uint64_t* __restrict__ keys, int64_t n, int32_t max_occ, unsigned long long* __restrict__ stats)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool first = false, over = false;
    if (i < n) {
        const uint64_t key = keys[i];
        first = i == 0 || keys[i - 1] != key;
        // the (max_occ + 1)-th entry of a run: one per key with more than max_occ entries
        over = i >= max_occ && keys[i - max_occ] == key && (i == max_occ || keys[i - max_occ - 1] != key);
    }
    const int nf = __popcll(__ballot(first)), no = __popcll(__ballot(over));
    if ((threadIdx.x & 63) == 0) {          // sums only: their order reaches nothing
        if (nf) atomicAdd(&stats[0], (unsigned long long)nf);
        if (no) atomicAdd(&stats[1], (unsigned long long)no);
    }
}

hipError_t launch_seed_index_stats(const uint64_t* keys, int64_t n, int32_t max_occ, unsigned long long* stats, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(seed_index_stats_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, keys, n, max_occ, stats);
    return hipGetLastError();
}

// first index in [0, n) whose key is >= (UPPER: >) key
template <bool UPPER>
__device__ __forceinline__ int64_t sd_bound(const uint64_t* __restrict__ keys, int64_t n, uint64_t key)
{
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        const uint64_t v = keys[mid];
        if (UPPER ? v <= key : v < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(256) seed_lookup_kernel(const uint64_t* __restrict__ idx_keys, int64_t n_idx, int32_t max_occ, const uint64_t* __restrict__ rkeys,
                                                          int64_t nmin, int64_t* __restrict__ lo, int32_t* __restrict__ cnt, uint8_t* __restrict__ rep)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= nmin) return;
    const uint64_t key = rkeys[e];
    const int64_t a = sd_bound<false>(idx_keys, n_idx, key), b = sd_bound<true>(idx_keys, n_idx, key);
    const int64_t occ = b - a;
    lo[e] = a;
    cnt[e] = occ > max_occ ? 0 : (int32_t)occ;
    rep[e] = occ > max_occ ? 1 : 0;
}

hipError_t launch_seed_lookup(const uint64_t* idx_keys, int64_t n_idx, int32_t max_occ, const uint64_t* rkeys, int64_t nmin, int64_t* lo, int32_t* cnt, uint8_t* rep,
                              hipStream_t stream)
{
    if (nmin <= 0) return hipSuccess;
    hipLaunchKernelGGL(seed_lookup_kernel, dim3((unsigned)((nmin + 255) / 256)), dim3(256), 0, stream, idx_keys, n_idx, max_occ, rkeys, nmin, lo, cnt, rep);
    return hipGetLastError();
}

__global__ void __launch_bounds__(256) seed_per_read_kernel(const int64_t* __restrict__ seq_item0, const int64_t* __restrict__ item_off, const int64_t* __restrict__ aoff,
                                                            const uint8_t* __restrict__ rep, int32_t n, int64_t* __restrict__ read_moff, int64_t* __restrict__ read_aoff,
                                                            int32_t* __restrict__ repetitive)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r > n) return;
    const int64_t m0 = item_off[seq_item0[r]];
    read_moff[r] = m0;
    read_aoff[r] = aoff[m0];
    if (r == n) return;
    const int64_t m1 = item_off[seq_item0[r + 1]];
    int c = 0;
    for (int64_t e = m0; e < m1; ++e) c += rep[e];
    repetitive[r] = c;
}

hipError_t launch_seed_per_read(const int64_t* seq_item0, const int64_t* item_off, const int64_t* aoff, const uint8_t* rep, int32_t n, int64_t* read_moff,
                                int64_t* read_aoff, int32_t* repetitive, hipStream_t stream)
{
    hipLaunchKernelGGL(seed_per_read_kernel, dim3((unsigned)((n + 1 + 255) / 256)), dim3(256), 0, stream, seq_item0, item_off, aoff, rep, n, read_moff, read_aoff, repetitive);
    return hipGetLastError();
}

__global__ void __launch_bounds__(256) seed_anchor_fill_kernel(const uint64_t* __restrict__ idx_vals, int64_t n_idx, const uint64_t* __restrict__ rvals,
                                                               const int32_t* __restrict__ seq_of, const int64_t* __restrict__ read_len, const int64_t* __restrict__ lo,
                                                               const int32_t* __restrict__ cnt, const int64_t* __restrict__ aoff, int64_t m0, int64_t m1, int64_t a0,
                                                               int32_t k, uint64_t* __restrict__ k1, uint64_t* __restrict__ k2, int64_t cap)
{
    const int64_t e = m0 + (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= m1) return;
    const int c = cnt[e];
    if (c <= 0) return;
    const uint64_t rv = rvals[e];
    const int64_t q = (int64_t)(rv >> 1), first = lo[e], out = aoff[e] - a0;
    const uint64_t r = (uint64_t)(uint32_t)seq_of[e];
    const int64_t L = read_len[r];
    for (int t = 0; t < c; ++t) {
        const int64_t at = first + t, a = out + t;
        if (at < 0 || at >= n_idx || a < 0 || a >= cap) break;
        const uint64_t iv = idx_vals[at];
        const uint64_t minus = (rv ^ iv) & 1;
        const int64_t y = minus ? L - k - q : q;
        k1[a] = (r << 1) | minus;
        k2[a] = ((iv >> 1) << kSdYBits) | (uint64_t)y;
    }
}

hipError_t launch_seed_anchor_fill(const uint64_t* idx_vals, int64_t n_idx, const uint64_t* rvals, const int32_t* seq_of, const int64_t* read_len, const int64_t* lo,
                                   const int32_t* cnt, const int64_t* aoff, int64_t m0, int64_t m1, int64_t a0, int32_t k, uint64_t* k1, uint64_t* k2, int64_t cap,
                                   hipStream_t stream)
{
    if (m1 <= m0 || cap <= 0) return hipSuccess;
    hipLaunchKernelGGL(seed_anchor_fill_kernel, dim3((unsigned)((m1 - m0 + 255) / 256)), dim3(256), 0, stream, idx_vals, n_idx, rvals, seq_of, read_len, lo, cnt, aoff, m0,
                       m1, a0, k, k1, k2, cap);
    return hipGetLastError();
}

__global__ void __launch_bounds__(256) seed_segments_kernel(ChParams c)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s > c.nseg) return;
    c.seg_bounds[s] = sd_bound<false>(c.k1, c.n_anchors, (uint64_t)c.read0 * 2 + (uint64_t)s);
}

hipError_t launch_seed_segments(const ChParams& c, hipStream_t stream)
{
    hipLaunchKernelGGL(seed_segments_kernel, dim3((unsigned)((c.nseg + 1 + 255) / 256)), dim3(256), 0, stream, c);
    return hipGetLastError();
}

__device__ __forceinline__ int64_t wave_max(int64_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const int64_t o = __shfl_xor(v, d);
        v = o > v ? o : v;
    }
    return v;
}

// Between an LDS write and the reads of it by other lanes of the SAME wave: a wave's LDS operations execute in issue order, so all that is
// needed is that the compiler keeps them in program order.  seed_chain_kernel is one wave per workgroup (its launch bounds), so this stands
// where a workgroup barrier would, without the barrier's wait for the global stores in flight.
__device__ __forceinline__ void wave_lds_order()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// contig of the genome-wide position x, or -1
__device__ __forceinline__ int ch_contig(const ChParams& c, int64_t x)
{
    int lo = 0, hi = c.n_contigs;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (c.ctg_off[mid] <= x) lo = mid + 1; else hi = mid;
    }
    const int g = lo - 1;
    return g >= 0 && x < c.ctg_off[g] + c.ctg_len[g] ? g : -1;
}

__global__ void __launch_bounds__(64) seed_chain_kernel(ChParams c)
{
    __shared__ int64_t rx[64];
    __shared__ int32_t ry[64], rf[64], rc[64];
    const int s = blockIdx.x, lane = threadIdx.x;
    int64_t* seg = c.seg + (int64_t)s * kChSeg;
    const int64_t a0 = c.seg_bounds[s], a1 = c.seg_bounds[s + 1];
    if (a0 < 0 || a1 < a0 || a1 > c.n_anchors || a1 - a0 > 0x7fffffff) {
        if (lane == 0) { seg[0] = 0; seg[1] = 0; seg[2] = 0; seg[3] = 2; }
        return;
    }
    const int A = (int)(a1 - a0);
    const uint64_t* k2 = c.k2 + a0;
    int32_t* f = c.f + a0;
    int32_t* p = c.p + a0;
    uint8_t* used = c.used + a0;
    const int k = c.k;
    const int64_t none = INT64_MIN;
    int ci = -1;                                         // the contig of the anchor before, [c_lo, c_hi): searched again only when x leaves it
    int64_t c_lo = 0, c_hi = 0;
    uint64_t w2 = A > 0 ? k2[0] : 0;
    for (int i = 0; i < A; ++i) {
        const uint64_t w2_next = i + 1 < A ? k2[i + 1] : 0;     // asked for one anchor ahead
        const int64_t xi = (int64_t)(w2 >> kSdYBits);
        const int32_t yi = (int32_t)(w2 & (((uint64_t)1 << kSdYBits) - 1));
        if (xi < c_lo || xi >= c_hi) {
            ci = ch_contig(c, xi);
            c_lo = ci >= 0 ? c.ctg_off[ci] : 0;
            c_hi = ci >= 0 ? c_lo + c.ctg_len[ci] : 0;
        }
        const int j = i - 1 - lane;
        int64_t cand = none;
        if (lane < c.lookback && j >= 0) {
            const int slot = j & 63;
            const int64_t dx = xi - rx[slot], dy = (int64_t)yi - ry[slot];
            const int64_t skew = dx > dy ? dx - dy : dy - dx;
            if (rc[slot] == ci && dx > 0 && dy > 0 && dx <= c.max_gap && dy <= c.max_gap && skew <= c.max_skew)
                cand = (rf[slot] + ch_gain(dx, dy, k)) * 64 + (int64_t)(63 - lane);      // the value may be negative: no shift of it
        }
        const int64_t best = wave_max(cand);
        int32_t fi = k, pi = -1;
        if (best != none && (best >> 6) > k) { fi = (int32_t)(best >> 6); pi = i - 1 - (63 - (int)(best & 63)); }
        f[i] = fi; p[i] = pi; used[i] = 0;               // every lane stores the same: each lane reads back only what it wrote itself
        wave_lds_order();                                // slot i & 63 held anchor i - 64, which lane 63 has just read
        if (lane == 0) { rx[i & 63] = xi; ry[i & 63] = yi; rf[i & 63] = fi; rc[i & 63] = ci; }
        wave_lds_order();
        w2 = w2_next;
    }
    int emitted = 0, attempts = 0, truncated = 0, status = 0;
    while (emitted < c.max_chains) {
        int64_t cand = -1;
        for (int i = lane; i < A; i += 64)
            if (!used[i]) { const int64_t v = ((int64_t)f[i] << 31) | (int64_t)(0x7fffffff - i); cand = v > cand ? v : cand; }
        const int64_t best = wave_max(cand);
        if (best < 0) break;
        const int32_t fe = (int32_t)(best >> 31);
        const int e = 0x7fffffff - (int)(best & 0x7fffffff);
        if (fe < c.min_score) break;
        if (attempts >= c.max_attempts) { truncated = 1; break; }
        ++attempts;
        int i = e, count = 0, first = e;
        for (int step = 0; step < A && i >= 0 && !used[i]; ++step) {
            used[i] = 1; ++count; first = i;
            int pi = p[i];
            if (pi < -1 || pi >= i) { status = 3; pi = -1; }     // never followed outside [0, i)
            i = pi;
        }
        const int32_t score = fe - (i >= 0 ? f[i] : 0);
        if (score >= c.min_score && count >= c.min_anchors) {
            const uint64_t wf = k2[first], wl = k2[e];
            const int64_t xf = (int64_t)(wf >> kSdYBits), xl = (int64_t)(wl >> kSdYBits);
            const int g = ch_contig(c, xl);
            const int64_t g0 = g >= 0 ? c.ctg_off[g] : 0;
            if (lane == 0) {
                int64_t* row = c.rows + ((int64_t)s * c.max_chains + emitted) * kChRow;
                row[0] = c.read0 + (s >> 1); row[1] = s & 1; row[2] = g; row[3] = score; row[4] = count;
                row[5] = xf - g0; row[6] = (int64_t)(wf & (((uint64_t)1 << kSdYBits) - 1));
                row[7] = xl - g0 + k; row[8] = (int64_t)(wl & (((uint64_t)1 << kSdYBits) - 1)) + k; row[9] = 0;
            }
            ++emitted;
        }
    }
    if (lane == 0) { seg[0] = emitted; seg[1] = truncated; seg[2] = A; seg[3] = status; }
}

hipError_t launch_seed_chain(const ChParams& c, hipStream_t stream)
{
    if (c.nseg <= 0) return hipSuccess;
    hipLaunchKernelGGL(seed_chain_kernel, dim3((unsigned)c.nseg), dim3(64), 0, stream, c);
    return hipGetLastError();
}

}  // namespace clh
