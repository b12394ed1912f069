// seed_circle.hip -- K7c: the circles of a read batch in one device pass.  What stands between the link kernel (seed_link.hip) and the
// junction kernel (seed_junction.hip), and behind the latter: the best path of every read, its K7j tasks and their class routing, the
// winner among the refined junctions with its flanking dinucleotides, and the table of the distinct circles with their read counts.
// Definitions: seed_device.h (cc_tie_key, cc_path_before, cc_task, cc_task_ok, cc_ordinal, cc_winner, cc_flanks, cc_read_pos),
// include/ciri_long_hip.h and DESIGN.md section 4 (K7c); the plain statement is tests/circle_check.py.
//
// seed_circle_select_kernel: one wave per read, lane l holds chain l of the plus and of the minus segment (seed_link.hip's geometry, no
// LDS).  Every lane reduces its own candidates (a chain with pos == 0 whose path scores at least min_path_score) to one (score, tie key)
// pair and one butterfly over the pair picks the least under (-score, minus, x_first, path).  The chains of that path are the lanes whose
// path index equals the winner's; those of kind 3 set bit `pos` of a wave-wide mask and a link's ordinal is the number of set bits below
// its own.  The chain and the link kernel's status words and the rows' marker words are checked as sd_seeds checks them on the host for
// clh_seed_link_batch; every index taken from a row (path, pos, pred, contig) is checked against its range before it is used, every task against
// what clh_seed_junction_batch admits; a read that fails is marked kCcBad, builds no task, and its circle row stays unwritten.
// A read's tasks go to its own slots, [r slots, r slots + links), so that nothing is counted twice and no offset has to be known first.
//
// seed_circle_route_kernel: one lane per slot; the filled slots are appended to their class's stretch of `order` (the stretches start at
// the prefix sums of count[], which the select kernel filled).  The order inside a class is that of arrival and changes nothing: a task's
// row depends on the task alone.
//
// seed_circle_finalise_kernel: one lane per read: cc_winner over its K7j rows, the four flank letters from the resident genome, the row.
//
// The table: key words per read, two stable least-significant-first sorts ((end, strand), then (contig, start) with the rows of
// another status last), head flags, the exclusive scan of seed_sort.hip, and a scatter whose counts and maxima are integer atomics
// (order-independent).  The stable sorts start from ascending reads, so a group's head is its lowest read.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "seed_device.h"

namespace clh {

__device__ __forceinline__ uint64_t cc_wave_or(uint64_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v |= (uint64_t)__shfl_xor((unsigned long long)v, d);
    return v;
}

__global__ void __launch_bounds__(64 * kCcWaves) seed_circle_select_kernel(CcLaunch L)
{
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * kCcWaves + (threadIdx.x >> 6);
    if (r >= L.nreads) return;
    int64_t* sel = L.sel + r * kCcSel;
    int32_t* cls = L.cls + r * L.slots;
    const int64_t read = (int64_t)L.read0 + r, RL = L.read_off[read + 1] - L.read_off[read];

    // the lane's chain of either segment
    int n[2], kind[2] = {0, 0}, pred[2] = {-1, -1}, path[2] = {-1, -1}, pos[2] = {-1, -1};
    bool bad = false;
    int64_t my_score = kCcNoScore;
    uint64_t my_key = ~(uint64_t)0;
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        const int64_t s = 2 * r + m;
        const int64_t nl = L.lseg[s * kLkSeg], nc = L.seg[s * kChSeg];
        n[m] = 0;
        if (nl != nc || nl < 0 || nl > L.max_chains || nl > 64 || L.lseg[s * kLkSeg + 3] != 0 || L.seg[s * kChSeg + 3] != 0) {     // unwritten, or a status of the chain or the link kernel
            bad = true;
            continue;
        }
        n[m] = (int)nl;
        if (lane >= n[m]) continue;
        const int64_t* lr = L.lrows + (s * L.max_chains + lane) * kLkRow;
        const int64_t* cr = L.rows + (s * L.max_chains + lane) * kChRow;
        const int64_t x0 = cr[5];
        if (cr[9] != 0 || lr[7] != 0 || lr[2] < -1 || lr[2] >= nl || lr[3] < 0 || lr[3] > 3 || lr[4] < 0 || lr[4] >= nl || lr[5] < 0 || lr[5] >= nl || x0 < 0 || x0 >= kLkLimit) {
            bad = true;
            continue;
        }
        kind[m] = (int)lr[3]; pred[m] = (int)lr[2]; path[m] = (int)lr[4]; pos[m] = (int)lr[5];
        if (pos[m] == 0 && lr[6] >= L.min_path_score) {
            const uint64_t kc = cc_tie_key(m, x0, path[m]);
            if (my_score == kCcNoScore || cc_path_before(lr[6], kc, my_score, my_key)) { my_score = lr[6]; my_key = kc; }
        }
    }
    bad = __any(bad);
    // the least under (-score, minus, x_first, path): one butterfly over the pair; a lane without a candidate loses to every other
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const int64_t os = __shfl_xor(my_score, d);
        const uint64_t ok = (uint64_t)__shfl_xor((unsigned long long)my_key, d);
        const bool take = os != kCcNoScore && (my_score == kCcNoScore || cc_path_before(os, ok, my_score, my_key));
        my_score = take ? os : my_score;
        my_key = take ? ok : my_key;
    }
    if (bad || my_score == kCcNoScore) {
        for (int o = lane; o < L.slots; o += 64) cls[o] = -1;
        if (lane == 0) {
            sel[0] = bad ? kCcBad : kCcNoPath;
#pragma unroll
            for (int f = 1; f < kCcSel; ++f) sel[f] = 0;
        }
        return;
    }
    const int minus = (int)(my_key >> 46) & 1, best = (int)(my_key & 63);
    const int nm = minus ? n[1] : n[0];
    const int kd = minus ? kind[1] : kind[0], pd = minus ? pred[1] : pred[0], pt = minus ? path[1] : path[0], ps = minus ? pos[1] : pos[0];
    const bool in_path = lane < nm && pt == best;
    const bool link = in_path && kd == kLkBacksplice;
    const int chains = __popcll(__ballot(in_path));
    const uint64_t mask = cc_wave_or(link ? (uint64_t)1 << ps : 0);
    const int links = __popcll(mask);
    int64_t task[kJxTask];
    int ordinal = 0, cl = 0;
    bool wrong = false;
    if (link) {
        ordinal = cc_ordinal(mask, ps);
        const int64_t s = 2 * r + minus;
        if (pd < 0 || pd >= nm || ordinal >= L.slots) wrong = true;                 // a back-splice without a source, or more links than chains
        else {
            cc_task(read, minus, L.rows + (s * L.max_chains + pd) * kChRow, L.rows + (s * L.max_chains + lane) * kChRow, L.k, task);
            if (task[2] < 0 || task[2] >= L.n_contigs || !cc_task_ok(task, RL, L.ctg_len[task[2]])) wrong = true;
            else cl = jx_status(task[3], task[4], task[5], task[6], L.max_span) ? 0 : jx_class(task[6] - task[4]);
        }
    }
    wrong = __any(wrong) || links != __popcll(__ballot(link));                      // two chains of one path at one pos
    if (link && !wrong) {
        int64_t* out = L.task + (r * L.slots + ordinal) * kJxTask;
#pragma unroll
        for (int f = 0; f < kJxTask; ++f) out[f] = task[f];
        cls[ordinal] = cl;
        atomicAdd(L.count + cl, 1ull);
    }
    for (int o = (wrong ? 0 : links) + lane; o < L.slots; o += 64) cls[o] = -1;     // the empty slots; no slot is written twice
    if (lane == 0) {
        sel[0] = wrong ? kCcBad : links ? kCcFound : kCcNoBacksplice;
        sel[1] = minus; sel[2] = my_score; sel[3] = chains; sel[4] = wrong ? 0 : links; sel[5] = 0; sel[6] = 0; sel[7] = 0;
    }
}

__global__ void __launch_bounds__(256) seed_circle_route_kernel(CcLaunch L)
{
    const int64_t slot = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (slot >= (int64_t)L.nreads * L.slots) return;
    const int c = L.cls[slot];
    if (c < 0 || c >= kJxClasses) return;
    unsigned long long base = 0;
    for (int b = 0; b < c; ++b) base += L.count[b];
    const unsigned long long at = base + atomicAdd(L.count + kJxClasses + c, 1ull);
    if (at < (unsigned long long)L.nreads * (unsigned long long)L.slots) L.order[at] = slot;
}

__global__ void __launch_bounds__(256) seed_circle_finalise_kernel(CcLaunch L)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= L.nreads) return;
    const int64_t* sel = L.sel + r * kCcSel;
    const int64_t read = (int64_t)L.read0 + r, RL = L.read_off[read + 1] - L.read_off[read];
    int64_t row[kCcRow];
#pragma unroll
    for (int f = 0; f < kCcRow; ++f) row[f] = 0;
    const int64_t state = sel[0];
    if (state != kCcFound && state != kCcNoPath && state != kCcNoBacksplice) return;         // kCcBad or unwritten: the row stays unwritten
    row[0] = state;
    if (state != kCcNoPath) { row[9] = sel[1]; row[10] = sel[2]; row[11] = sel[3]; row[12] = sel[4]; }
    if (state == kCcFound) {
        const int cnt = (int)sel[4];
        if (cnt < 1 || cnt > L.slots) return;
        const int64_t* jr = L.junction + r * L.slots * kJxRow;
        for (int t = 0; t < cnt; ++t)
            if (jr[(int64_t)t * kJxRow] < 0 || jr[(int64_t)t * kJxRow] > 2) return;          // a row K7j left unwritten
        int refined = 0;
        const int w = cc_winner(jr, cnt, &refined);
        row[13] = refined;
        if (w < 0) row[0] = kCcNoJunction;
        else {
            const int64_t* tk = L.task + (r * L.slots + w) * kJxTask;
            const int64_t* j = jr + (int64_t)w * kJxRow;
            const int64_t c = tk[2], end = j[6], start = j[7];
            if (c < 0 || c >= L.n_contigs) return;
            const int64_t off = L.ctg_off[c], len = L.ctg_len[c];
            if (start < 0 || start >= end || end > len || j[3] < 0 || j[3] > tk[6] - tk[4]) return;
            int donor, acceptor;
            cc_flanks(L.genome, off, len, start, end, j[2] != 0, &donor, &acceptor);
            row[1] = c; row[2] = start; row[3] = end; row[4] = j[2] != 0; row[5] = donor; row[6] = acceptor; row[7] = j[1];
            row[8] = cc_read_pos(RL, tk[4], j[3], tk[1] != 0); row[14] = w;
        }
    }
    int64_t* out = L.circle + read * kCcRow;
#pragma unroll
    for (int f = 0; f < kCcRow; ++f) out[f] = row[f];
}

hipError_t launch_seed_circle_select(const CcLaunch& l, hipStream_t stream)
{
    if (l.nreads <= 0) return hipSuccess;
    hipLaunchKernelGGL(seed_circle_select_kernel, dim3((unsigned)((l.nreads + kCcWaves - 1) / kCcWaves)), dim3(64 * kCcWaves), 0, stream, l);
    return hipGetLastError();
}

hipError_t launch_seed_circle_route(const CcLaunch& l, hipStream_t stream)
{
    const int64_t n = (int64_t)l.nreads * l.slots;
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(seed_circle_route_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, l);
    return hipGetLastError();
}

hipError_t launch_seed_circle_finalise(const CcLaunch& l, hipStream_t stream)
{
    if (l.nreads <= 0) return hipSuccess;
    hipLaunchKernelGGL(seed_circle_finalise_kernel, dim3((unsigned)((l.nreads + 255) / 256)), dim3(256), 0, stream, l);
    return hipGetLastError();
}

// ---- the table ------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool cc_same_circle(const int64_t* a, const int64_t* b) { return a[1] == b[1] && a[2] == b[2] && a[3] == b[3] && a[4] == b[4]; }

__global__ void __launch_bounds__(256) seed_circle_keys_kernel(const int64_t* circle, int64_t n, uint64_t* key_lo, uint64_t* key_hi, uint64_t* read)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t* c = circle + i * kCcRow;
    const bool found = c[0] == kCcFound;
    key_lo[i] = found ? ((uint64_t)c[3] << 1) | (uint64_t)(c[4] != 0) : 0;                   // end in [0, 2^40]
    key_hi[i] = found ? ((uint64_t)c[1] << 40) | (uint64_t)c[2] : (uint64_t)1 << 63;          // contig below 2^23, start below 2^40
    read[i] = (uint64_t)i;
}

__global__ void __launch_bounds__(256) seed_circle_gather_kernel(const uint64_t* key_hi, const uint64_t* perm, int64_t n, uint64_t* out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint64_t r = perm[i];
    out[i] = r < (uint64_t)n ? key_hi[r] : (uint64_t)1 << 63;
}

__global__ void __launch_bounds__(256) seed_circle_heads_kernel(const int64_t* circle, const uint64_t* perm, int64_t n, int32_t* head)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > n) return;
    int h = 0;
    if (i < n && perm[i] < (uint64_t)n) {
        const int64_t* c = circle + (int64_t)perm[i] * kCcRow;
        if (c[0] == kCcFound) h = i == 0 || perm[i - 1] >= (uint64_t)n || !cc_same_circle(c, circle + (int64_t)perm[i - 1] * kCcRow);
    }
    head[i] = h;                                        // head[n] = 0: first[n] is the number of circles
}

// heads write their group's row, the rest is added by the second kernel: counts and maxima are integer atomics
__global__ void __launch_bounds__(256) seed_circle_table_heads_kernel(const int64_t* circle, const uint64_t* perm, const int32_t* head, const int64_t* first, int64_t n,
                                                                      int64_t* table)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !head[i] || perm[i] >= (uint64_t)n) return;
    const int64_t g = first[i];
    if (g < 0 || g >= n) return;
    const int64_t* c = circle + (int64_t)perm[i] * kCcRow;
    int64_t* t = table + g * kCcTable;
    t[0] = c[1]; t[1] = c[2]; t[2] = c[3]; t[3] = c[4]; t[4] = c[5]; t[5] = c[6]; t[6] = 0; t[7] = INT64_MIN; t[8] = (int64_t)perm[i]; t[9] = 0;
}

__global__ void __launch_bounds__(256) seed_circle_table_members_kernel(const int64_t* circle, const uint64_t* perm, const int32_t* head, const int64_t* first, int64_t n,
                                                                        int64_t* table, int64_t* circle_of_read)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || perm[i] >= (uint64_t)n) return;
    const int64_t r = (int64_t)perm[i];
    const int64_t* c = circle + r * kCcRow;
    const int64_t g = first[i] + head[i] - 1;           // the heads up to and with this row, less one
    if (c[0] != kCcFound || g < 0 || g >= n) { circle_of_read[r] = -1; return; }
    circle_of_read[r] = g;
    atomicAdd((unsigned long long*)(table + g * kCcTable + 6), 1ull);
    atomicMax((long long*)(table + g * kCcTable + 7), (long long)c[7]);
}

hipError_t launch_seed_circle_keys(const int64_t* circle, int64_t n, uint64_t* key_lo, uint64_t* key_hi, uint64_t* read, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(seed_circle_keys_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, circle, n, key_lo, key_hi, read);
    return hipGetLastError();
}

hipError_t launch_seed_circle_gather(const uint64_t* key_hi, const uint64_t* perm, int64_t n, uint64_t* out, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(seed_circle_gather_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, key_hi, perm, n, out);
    return hipGetLastError();
}

hipError_t launch_seed_circle_heads(const int64_t* circle, const uint64_t* perm, int64_t n, int32_t* head, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(seed_circle_heads_kernel, dim3((unsigned)((n + 1 + 255) / 256)), dim3(256), 0, stream, circle, perm, n, head);
    return hipGetLastError();
}

hipError_t launch_seed_circle_table(const int64_t* circle, const uint64_t* perm, const int32_t* head, const int64_t* first, int64_t n, int64_t* table,
                                    int64_t* circle_of_read, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(seed_circle_table_heads_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, circle, perm, head, first, n, table);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(seed_circle_table_members_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, circle, perm, head, first, n, table, circle_of_read);
    return hipGetLastError();
}

}  // namespace clh
