// edit_search.hip -- K4s: short probes against whole texts, edlib's HW mode with task "locations", segmented on the device (gfx950).
//
// What it serves: adapter, primer and junction-probe searches -- a handful of probes of at most 64 letters, each searched in
// every text of a batch.  The pair route (edit_align.hip) wants the cross product written out and walks one pair's target as
// one dependent chain in one lane.  Here the texts are uploaded once, one wave takes one (probe, text) cell, and its 64 lanes
// walk 64 column segments of the text at the same time:
//   lane l of round r owns the columns [(64 r + l) SEG, (64 r + l + 1) SEG) and starts its recurrence 2 m columns earlier
//   (clamped at 0) from the HW initial state: top row 0, Pv all ones, score m.
// Exactness: an alignment of cost d covers at most m + d target columns and the best cost at any column is at most m, so every
// alignment that decides the last-row value of an owned column starts inside the warm-up; the fresh start can only raise
// values.  The last-row value at every owned column is therefore that of the full run.  Warm-up columns are walked and never
// counted.  Each lane keeps (best, first column, last column, count) over its owned columns; lanes, rounds and chunks join by
// the minimum best and, among its holders, the minimum first, the maximum last and the sum of the counts, seeded with column
// -1 at score m.  The start of the first location is align's rule: one SHW pass of the reversed probe over the reversed
// text[.. end], at most m + best + 1 columns.  tools/edit_search_model.py states all of it in Python.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include "clh_device.h"

namespace clh {

template <int W> struct EsWord;
template <> struct EsWord<32> { typedef unsigned int T; };
template <> struct EsWord<64> { typedef unsigned long long T; };

struct EsBest { int best, first, last, cnt; };

__device__ __forceinline__ void es_join(EsBest& a, int best, int first, int last, int cnt)
{
    if (best < a.best) { a.best = best; a.first = first; a.last = last; a.cnt = cnt; }
    else if (best == a.best) { a.first = min(a.first, first); a.last = max(a.last, last); a.cnt += cnt; }
}

__device__ __forceinline__ void es_wave_join(EsBest& b)
{
    for (int off = 32; off > 0; off >>= 1) {
        const int best = __shfl_xor(b.best, off), first = __shfl_xor(b.first, off), last = __shfl_xor(b.last, off), cnt = __shfl_xor(b.cnt, off);
        es_join(b, best, first, last, cnt);
    }
}

__device__ __forceinline__ unsigned int es_rev(unsigned int x, int m) { return __brev(x) >> (32 - m); }
__device__ __forceinline__ unsigned long long es_rev(unsigned long long x, int m) { return __brevll(x) >> (64 - m); }

// one column of Myers/Hyyro on one word; HIN: the horizontal delta entering row 0 (0 HW, 1 SHW) -> the last row's delta
template <typename T, int HIN>
__device__ __forceinline__ int es_step(T Eq, T& Pv, T& Mv, int lb)
{
    const T Xv = Eq | Mv;
    const T Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
    T Ph = Mv | ~(Xh | Pv);
    T Mh = Pv & Xh;
    const int d = (int)((Ph >> lb) & 1) - (int)((Mh >> lb) & 1);
    Ph = (Ph << 1) | (T)HIN;
    Mh <<= 1;
    Pv = Mh | ~(Xv | Ph);
    Mv = Ph & Xv;
    return d;
}

__device__ __forceinline__ void es_track(EsBest& b, int score, int col)
{
    const bool lt = score < b.best, le = score <= b.best;
    b.first = lt ? col : b.first;
    b.last = le ? col : b.last;
    b.cnt = lt ? 1 : b.cnt + (le ? 1 : 0);
    b.best = lt ? score : b.best;
}

// the columns [c0, c1) of one lane, eight text bytes per load where eight are left (never a byte outside [c0, c1))
template <typename T, bool TRACK>
__device__ __forceinline__ void es_walk(const uint8_t* __restrict__ txt, int c0, int c1, const T* peq, int lb, T& Pv, T& Mv, int& score, EsBest& b)
{
    int col = c0;
    for (; col + 8 <= c1; col += 8) {
        unsigned long long w;
        __builtin_memcpy(&w, txt + col, 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            score += es_step<T, 0>(peq[(unsigned int)(w >> (8 * j)) & 255u], Pv, Mv, lb);
            if (TRACK) es_track(b, score, col + j);
        }
    }
    for (; col < c1; ++col) {
        score += es_step<T, 0>(peq[txt[col]], Pv, Mv, lb);
        if (TRACK) es_track(b, score, col);
    }
}

// The wave's 256 match masks in LDS, the additional equalities OR-ed in (symmetric, not transitive, on the letters as given).
// Every wave of the workgroup passes both barriers, with or without a cell.
template <typename T>
__device__ __forceinline__ void es_build_peq(T* peq, const uint8_t* __restrict__ pat, int m, const uint8_t* __restrict__ eq, int n_eq, int lane)
{
    for (int i = lane; i < 256; i += 64) peq[i] = 0;
    __syncthreads();
    if (lane < m) {
        const int c = pat[lane];
        const T bit = (T)1 << lane;
        atomicOr(&peq[c], bit);
        for (int e = 0; e < n_eq; ++e) {
            const int a = eq[2 * e], b = eq[2 * e + 1];
            if (c == a) atomicOr(&peq[b], bit);
            if (c == b) atomicOr(&peq[a], bit);
        }
    }
    __syncthreads();
}

// the joined tuple of a cell -> its row.  Every lane of the wave runs the same bounded reverse pass; lane 0 stores.
template <typename T>
__device__ __forceinline__ void es_finish(const EsParams& p, EsBest b, const uint8_t* __restrict__ txt, const T* peq, int m, int64_t cell, int lane)
{
    es_join(b, m, -1, -1, 1);                               // column -1: the probe in front of the text
    int out[5] = {b.best, 0, b.first, b.last, b.cnt};
    if (p.k >= 0 && b.best > p.k) { out[0] = -1; out[1] = out[2] = out[3] = -2; out[4] = 0; }
    else if (b.first >= 0) {
        const int end = b.first, P = min(end + 1, m + b.best + 1);
        T Pv = ~(T)0, Mv = 0;
        int score = m, lastp = -1;
        for (int x = 0; x < P; ++x) {
            score += es_step<T, 1>(es_rev(peq[txt[end - x]], m), Pv, Mv, m - 1);
            if (score == b.best) lastp = x;
        }
        if (lastp < 0) return;                              // cannot happen; the row stays unwritten and fetch reports it
        out[1] = end - lastp;
    }
    if (lane == 0 && cell >= 0 && cell < p.ncell)
        for (int f = 0; f < 5; ++f) p.rows[cell * 5 + f] = out[f];
}

template <int W>
__global__ void __launch_bounds__(256) edit_search_kernel(EsParams p)
{
    typedef typename EsWord<W>::T T;
    __shared__ T peq_s[4][256];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    T* peq = peq_s[wv];
    const int64_t item = (int64_t)blockIdx.x * 4 + wv;
    const bool live = item < (int64_t)p.nlist * p.total_chunks;
    int probe = 0, m = 0;
    int64_t g = 0;
    if (live) {
        probe = p.probe_list[item / p.total_chunks];
        g = item % p.total_chunks;
        m = (int)(p.probe_off[probe + 1] - p.probe_off[probe]);
    }
    es_build_peq<T>(peq, p.probe + p.probe_off[probe], m, p.eq, p.n_eq, lane);
    if (!live) return;
    int lo = 0, hi = p.ntext;                               // the text of chunk g: the last one whose first chunk is at or before g
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (p.chunk_base[mid] <= g) lo = mid; else hi = mid; }
    const int t = lo;
    const int64_t toff = p.text_off[t];
    const int n = (int)(p.text_off[t + 1] - toff);
    const uint8_t* txt = p.text + toff;
    const int c = (int)(g - p.chunk_base[t]), nch = (int)(p.chunk_base[t + 1] - p.chunk_base[t]);
    EsBest b = {INT_MAX, INT_MAX, -2, 0};
    const int r1 = min((c + 1) * kEsChunkRounds, (n + kEsRound - 1) / kEsRound);
    for (int r = c * kEsChunkRounds; r < r1; ++r) {
        const int own0 = (r * 64 + lane) * kEsSeg;
        if (own0 >= n) continue;
        const int c0 = max(0, own0 - 2 * m), c1 = min(own0 + kEsSeg, n);
        T Pv = ~(T)0, Mv = 0;
        int score = m;
        es_walk<T, false>(txt, c0, own0, peq, m - 1, Pv, Mv, score, b);
        es_walk<T, true>(txt, own0, c1, peq, m - 1, Pv, Mv, score, b);
    }
    es_wave_join(b);
    if (nch == 1) { es_finish<T>(p, b, txt, peq, m, (int64_t)t * p.nprobe + probe, lane); return; }
    const int64_t at = (int64_t)probe * p.total_chunks + g;
    if (lane == 0 && at < p.npart) { p.part[at * 4] = b.best; p.part[at * 4 + 1] = b.first; p.part[at * 4 + 2] = b.last; p.part[at * 4 + 3] = b.cnt; }
}

// one wave per (probe, split text): joins the text's chunks and finishes the cell
template <int W>
__global__ void __launch_bounds__(256) edit_search_finish_kernel(EsParams p)
{
    typedef typename EsWord<W>::T T;
    __shared__ T peq_s[4][256];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    T* peq = peq_s[wv];
    const int64_t item = (int64_t)blockIdx.x * 4 + wv;
    const bool live = item < (int64_t)p.nlist * p.nsplit;
    int probe = 0, m = 0, t = 0;
    if (live) {
        probe = p.probe_list[item / p.nsplit];
        t = p.split_list[item % p.nsplit];
        m = (int)(p.probe_off[probe + 1] - p.probe_off[probe]);
    }
    es_build_peq<T>(peq, p.probe + p.probe_off[probe], m, p.eq, p.n_eq, lane);
    if (!live || t < 0 || t >= p.ntext) return;
    const int64_t g0 = p.chunk_base[t];
    const int nch = (int)(p.chunk_base[t + 1] - g0);
    EsBest b = {INT_MAX, INT_MAX, -2, 0};
    bool unwritten = false;
    for (int i = lane; i < nch; i += 64) {
        const int64_t at = (int64_t)probe * p.total_chunks + g0 + i;
        if (at >= p.npart) { unwritten = true; continue; }
        const int best = p.part[at * 4], first = p.part[at * 4 + 1], last = p.part[at * 4 + 2], cnt = p.part[at * 4 + 3];
        if (cnt == kEsUnwritten) unwritten = true;
        es_join(b, best, first, last, cnt);
    }
    if (__ballot(unwritten)) return;                        // a chunk without a tuple: the row stays unwritten and fetch reports it
    es_wave_join(b);
    es_finish<T>(p, b, p.text + p.text_off[t], peq, m, (int64_t)t * p.nprobe + probe, lane);
}

hipError_t launch_edit_search(const EsParams& p, int W, hipStream_t stream)
{
    const int64_t items = (int64_t)p.nlist * p.total_chunks;
    if (items <= 0) return hipSuccess;
    if ((items + 3) / 4 > INT_MAX) return hipErrorInvalidValue;
    const dim3 grid((unsigned int)((items + 3) / 4));
    if (W == 32) hipLaunchKernelGGL(edit_search_kernel<32>, grid, dim3(256), 0, stream, p);
    else hipLaunchKernelGGL(edit_search_kernel<64>, grid, dim3(256), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_edit_search_finish(const EsParams& p, int W, hipStream_t stream)
{
    const int64_t items = (int64_t)p.nlist * p.nsplit;
    if (items <= 0) return hipSuccess;
    if ((items + 3) / 4 > INT_MAX) return hipErrorInvalidValue;
    const dim3 grid((unsigned int)((items + 3) / 4));
    if (W == 32) hipLaunchKernelGGL(edit_search_finish_kernel<32>, grid, dim3(256), 0, stream, p);
    else hipLaunchKernelGGL(edit_search_finish_kernel<64>, grid, dim3(256), 0, stream, p);
    return hipGetLastError();
}

}  // namespace clh
