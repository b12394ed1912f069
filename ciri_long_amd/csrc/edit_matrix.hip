// edit_matrix.hip -- the work in front of K4 when whole groups of strings want all their pairs (gfx950).
//
// What it replaces: cluster_sequence (CIRI_long/collapse.py:458-473) homopolymer-compresses every read (utils.py:162-167) and
// calls distance(x, y) for every pair i < j of a list.  The pair form of K4 (clh_edit_plan_create) made the host write
// every pair out as two strings, so a list of 50 travelled 49 times.  Here the strings are uploaded once:
//   hpc_compress_kernel       homopolymer compression, one wave per string, into a second buffer at the same offsets;
//   edit_matrix_tasks_kernel  one thread per pair of every group: (i, j) from the pair's position in the condensed upper
//                             triangle (np.triu_indices(n, 1) order), the EdTask K4 wants, filed under its lane-group class.
// The tasks kernel runs twice: a counting pass, then a filling pass that places each class behind the classes before it,
// so one task array of npairs entries holds all classes back to back.  K4 itself (edit_distance.hip) is unchanged.
// tools/edit_matrix_model.py states the keep rule and the index inversion in Python.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "clh_device.h"

namespace clh {

// Byte i of a string is kept iff i == 0 or it differs from byte i-1 of the same string.  A step is 64 bytes, one per lane;
// the write position of a kept byte is the running length plus the kept bytes in lower lanes.  `kept` is wave-uniform.
__global__ void __launch_bounds__(256) hpc_compress_kernel(const uint8_t* __restrict__ raw, const int64_t* __restrict__ seq_off, int nseq,
                                                           uint8_t* __restrict__ hpc, int32_t* __restrict__ len)
{
    const int lane = threadIdx.x & 63;
    const int s = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= nseq) return;                                   // the whole wave leaves
    const int64_t off = seq_off[s];
    const int n = (int)(seq_off[s + 1] - off);
    const uint8_t* in = raw + off;
    uint8_t* out = hpc + off;                                // the string's own slot: the output never outgrows it
    int kept = 0;
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        const bool inside = i < n;
        const int c = inside ? in[i] : 0;
        const int before = inside && i > 0 ? in[i - 1] : -1;   // read from the string, also across a step's border
        const bool keep = inside && c != before;
        const unsigned long long m = __ballot(keep);
        if (keep) out[kept + __popcll(m & ((1ull << lane) - 1ull))] = (uint8_t)c;
        kept += __popcll(m);
    }
    if (lane == 0) len[s] = kept;
}

// position q of the condensed upper triangle of n items -> (i, j), i < j.  r = pairs behind q; row i = n-2-k holds q iff
// k (k + 1) / 2 <= r < (k + 1) (k + 2) / 2.  The square root only proposes k; the two loops make it exact.
__device__ __forceinline__ void em_pair_of(int64_t q, int64_t n, int* i, int* j)
{
    const int64_t r = n * (n - 1) / 2 - 1 - q;
    int64_t k = (int64_t)((sqrt((double)(8 * r + 1)) - 1.0) * 0.5);
    while (k > 0 && k * (k + 1) / 2 > r) --k;
    while ((k + 1) * (k + 2) / 2 <= r) ++k;
    const int64_t row = n - 2 - k;
    *i = (int)row;
    *j = (int)(q - row * (2 * n - row - 1) / 2 + row + 1);
}

// One thread per pair.  The per-class counters are bumped once per wave and class (a ballot finds the lanes of a class, the first of them
// adds their number and hands the base to the others): one add per pair on a single word is what bounds the kernel otherwise.
template <bool FILL>
__global__ void __launch_bounds__(256) edit_matrix_tasks_kernel(EmParams p)
{
    const int lane = threadIdx.x & 63;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int cls = -1;                                           // stays -1 for a thread without a task
    EdTask task;
    task.pat_off = 0; task.txt_off = 0; task.pat_len = 0; task.txt_len = 0; task.out_index = 0; task.carry_off64 = -1;
    if (t < p.npairs) {
        // the group: the last one whose first pair is at or before t (groups without pairs share their successor's base)
        int lo = 0, hi = p.ngroups;
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (p.pair_base[mid] <= t) lo = mid; else hi = mid; }
        const int64_t first = p.group_off[lo], n = p.group_off[lo + 1] - first;
        int i, j;
        em_pair_of(t - p.pair_base[lo], n, &i, &j);
        const int64_t a = first + i, b = first + j;
        const int la = p.len[a], lb = p.len[b];
        if (la == 0 || lb == 0) {
            if (FILL) p.out[t] = la + lb;
        } else {
            const bool a_is_pat = la <= lb;                 // K4 wants the shorter string as the pattern
            task.pat_off = p.seq_off[a_is_pat ? a : b]; task.txt_off = p.seq_off[a_is_pat ? b : a];
            task.pat_len = a_is_pat ? la : lb; task.txt_len = a_is_pat ? lb : la;
            task.out_index = (int32_t)t;
            const int B = (task.pat_len + 63) >> 6;
            cls = 0;
            while ((1 << cls) < B && cls < 6) ++cls;        // lane group G = 1 << cls, the rule of ed_group (clh_api.hip)
            if (FILL && task.pat_len > 4096) {              // two between-pass delta buffers of one byte per text column (+ slack), as K4 lays them out
                const unsigned long long need = 2ull * (((unsigned long long)task.txt_len + 63) / 64 + 1);
                const unsigned long long at = atomicAdd(&p.ctl->carry_used64, need);
                if (at + need > (unsigned long long)p.carry_cap64) { atomicAdd(&p.ctl->no_carry, 1u); p.out[t] = -1; task.pat_len = -1; }   // reported: the run fails
                else task.carry_off64 = (int32_t)at;
            }
        }
    }
    for (int c = 0; c < 7; ++c) {
        const unsigned long long m = __ballot(cls == c);
        if (m == 0) continue;                               // wave-uniform
        const int leader = __ffsll((long long)m) - 1;
        unsigned int base = 0;
        if (lane == leader) base = atomicAdd(FILL ? &p.ctl->fill[c] : &p.ctl->count[c], (unsigned int)__popcll(m));
        if (!FILL) continue;
        base = __shfl(base, leader);
        if (cls == c && task.pat_len > 0) {
            unsigned int at = base + __popcll(m & ((1ull << lane) - 1ull));
            for (int k = 0; k < c; ++k) at += p.ctl->count[k];
            p.tasks[at] = task;
        }
    }
}

hipError_t launch_hpc_compress(const uint8_t* raw, const int64_t* seq_off, int nseq, uint8_t* hpc, int32_t* len, hipStream_t stream)
{
    if (nseq <= 0) return hipSuccess;
    hipLaunchKernelGGL(hpc_compress_kernel, dim3((nseq + 3) / 4), dim3(256), 0, stream, raw, seq_off, nseq, hpc, len);
    return hipGetLastError();
}

hipError_t launch_edit_matrix_tasks(const EmParams& p, bool fill, hipStream_t stream)
{
    if (p.npairs <= 0) return hipSuccess;
    const dim3 grid((unsigned int)((p.npairs + 255) / 256));
    if (fill) hipLaunchKernelGGL(edit_matrix_tasks_kernel<true>, grid, dim3(256), 0, stream, p);
    else hipLaunchKernelGGL(edit_matrix_tasks_kernel<false>, grid, dim3(256), 0, stream, p);
    return hipGetLastError();
}

}  // namespace clh
