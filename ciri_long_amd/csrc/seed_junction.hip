// seed_junction.hip -- K7j: the back-splice junction of a link refined to the base.
// Definitions: seed_device.h (jx_status, jx_nd, jx_na, jx_letter, jx_site, jx_read_letter), include/ciri_long_hip.h and DESIGN.md
// section 4 (K7j); the plain statement is tests/junction_check.py.
//
// A task holds m = ya - yd read letters Q between two anchors and one unknown, the split t: Q[0:t) continues forward from the donor
// anchor (the letters D of the contig), Q[t:m) runs up to the acceptor anchor (the letters A).  J(s, t, u, v) = HL[t][u] + HR[t][v]
// - start_s(xd + u) - end_s(xa - v - 1) - intron_open, HL and HR global affine scores.  The two site costs are not coupled, so per
// strand s the maximum separates into BL_s[t] = max_u (HL[t][u] - start_s) and BR_s[t] = max_v (HR[t][v] - end_s).
//
// seed_junction_kernel<CPL>: one wave per task with K1g's roles swapped.  The lanes own the rows: lane l holds rows t = l CPL + 1 ..
// l CPL + CPL of the read in registers (CPL 1, 2, 4, 8 for m up to 64, 128, 256, 512; row 0 is the boundary and uniform), the loop
// runs over the contig's letters, 64 of them fetched at once, one per lane, with both strands' site costs of their columns, and
// handed to the wave one column at a time by readlane.  The gap that runs along the lanes is K1g's max-plus prefix scan in the frame
// F[t] + t ge (wave_prefix_max + one DPP move, exact because go >= ge lets T stand for H); the gap along the contig is lane-private.
// BL_s[t] is a lane-private running maximum of (H[t][u] - start_s(u)) 1024 + (1023 - u): one 32-bit key whose maximum is the greatest
// value at the smallest u (kJxBound in seed_device.h is what makes it fit).  No reduction across lanes happens per column.
// The right side is the same pass over the letters backwards from the acceptor anchor with the read letters backwards from ya; its
// row m - t stands in another lane than the left side's row t and is fetched once, at the end: for the lane's k-th row the wanted
// register index (m - k - 2) mod CPL is the same in every lane, so it is one select and one cross-lane read per row.  One butterfly
// on J 2048 + (strand +: 1024) + (1023 - t) picks strand + first, then the smallest t.  No LDS, nothing per task in global memory
// but its row; letters of the read and the genome are read in place, minus reads complemented as they are read.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "clh_device.h"
#include "clh_device_ops.h"
#include "seed_device.h"

namespace clh {

__device__ __forceinline__ int jx_max(int a, int b) { return a > b ? a : b; }

// the key of a value and an index part: value 1024 + part, the part in [0, 1023] (or a column's -cost 1024 + 1023 - column)
__device__ __forceinline__ int jx_key(int value, int index_part) { return (int)((uint32_t)value * (uint32_t)(1 << kJxIndexBits) + (uint32_t)index_part); }

// One side.  Column c = 1 .. n consumes contig letter x0 + dir (c - 1); the site of column c = 0 .. n is the dinucleotide at
// (p0 + dir c, p0 + dir c + 1), table part `part`.  q[k]: the read letter of row lane CPL + k + 1, 4 behind row m.
// -> Kp[k], Km[k]: the row's key for strand + and -, K0p, K0m those of row 0 (the same in every lane).
template <int CPL>
__device__ __forceinline__ void jx_side(const JxLaunch& L, int lane, const int (&q)[CPL], int n, int64_t coff, int64_t clen, int64_t x0, int dir, int64_t p0, int part,
                                        int (&Kp)[CPL], int (&Km)[CPL], int& K0p, int& K0m)
{
    const int go = L.go, ge = L.ge, match = L.match, miss = -L.mismatch;
    int H[CPL], E[CPL], off[CPL], poff[CPL];
    const int c0p = -jx_site(L.site, L.genome, coff, clen, p0, part, 0) * (1 << kJxIndexBits) + kJxIndexMask;
    const int c0m = -jx_site(L.site, L.genome, coff, clen, p0, part, 1) * (1 << kJxIndexBits) + kJxIndexMask;
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
        const int r = lane * CPL + k + 1;
        H[k] = -(go + (r - 1) * ge);
        E[k] = H[k] - go;                               // E of column 0 enters as H - go: the first E is H - go either way
        off[k] = -go + (r + 1) * ge;
        poff[k] = r * ge;
        Kp[k] = jx_key(H[k], c0p);
        Km[k] = jx_key(H[k], c0m);
    }
    K0p = c0p; K0m = c0m;                               // H[0][0] = 0
    for (int cb = 0; cb < n; cb += 64) {
        const int mine = cb + lane + 1;                 // the column whose letter and costs this lane fetches
        int lt = 5, kcp = 0, kcm = 0;
        if (mine <= n) {
            lt = jx_letter(L.genome, coff, clen, x0 + (int64_t)dir * (mine - 1));
            lt = lt > 3 ? 5 : lt;                       // equals no read letter
            const int64_t p = p0 + (int64_t)dir * mine;
            kcp = -jx_site(L.site, L.genome, coff, clen, p, part, 0) * (1 << kJxIndexBits) + (kJxIndexMask - mine);
            kcm = -jx_site(L.site, L.genome, coff, clen, p, part, 1) * (1 << kJxIndexBits) + (kJxIndexMask - mine);
        }
        const int cnt = n - cb < 64 ? n - cb : 64;
        for (int j = 0; j < cnt; ++j) {
            const int rc = __builtin_amdgcn_readlane(lt, j), cp = __builtin_amdgcn_readlane(kcp, j), cm = __builtin_amdgcn_readlane(kcm, j);
            const int c = cb + j + 1;
            const int h0prev = c > 1 ? -(go + (c - 2) * ge) : 0, h0 = -(go + (c - 1) * ge);      // H[0][c - 1], H[0][c]
            const int hleft = dpp_shr1(h0prev, H[CPL - 1]);                                      // H[first own row - 1][c - 1]
            int T[CPL], v = 0;
#pragma unroll
            for (int k = CPL - 1; k >= 0; --k) {        // downwards: H[k - 1] is still column c - 1's
                E[k] = jx_max(H[k] - go, E[k] - ge);
                const int d = (k ? H[k - 1] : hleft) + (q[k] == rc ? match : miss);
                T[k] = jx_max(d, E[k]);
                const int x = T[k] + off[k];
                v = k == CPL - 1 ? x : jx_max(v, x);
            }
            const int X0 = h0 - go + ge;                // row 0 in the frame
            v = lane == 0 ? jx_max(v, X0) : v;
            int u = dpp_shr1(X0, wave_prefix_max(v));   // lane 0 keeps X0
#pragma unroll
            for (int k = 0; k < CPL; ++k) {
                H[k] = jx_max(T[k], u - poff[k]);
                u = jx_max(u, T[k] + off[k]);
                Kp[k] = jx_max(Kp[k], jx_key(H[k], cp));
                Km[k] = jx_max(Km[k], jx_key(H[k], cm));
            }
            K0p = jx_max(K0p, jx_key(h0, cp));
            K0m = jx_max(K0m, jx_key(h0, cm));
        }
    }
}

// the key of row r (r >= 1: in lane (r - 1) / CPL, register kk = (r - 1) mod CPL, which the caller gives and is wave-uniform; r == 0: k0)
template <int CPL>
__device__ __forceinline__ int jx_row(const int (&K)[CPL], int k0, int r, int kk)
{
    int x = K[0];
#pragma unroll
    for (int j = 1; j < CPL; ++j) x = kk == j ? K[j] : x;
    const int y = __shfl(x, r > 0 ? (r - 1) / CPL : 0);
    return r > 0 ? y : k0;
}

__device__ __forceinline__ int64_t jx_wave_max(int64_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const int64_t o = __shfl_xor(v, d);
        v = o > v ? o : v;
    }
    return v;
}

template <int CPL>
__global__ void __launch_bounds__(64 * kJxWaves) seed_junction_kernel(JxLaunch L, int64_t first, int64_t last)
{
    const int lane = threadIdx.x & 63;
    const int64_t slot = first + (int64_t)blockIdx.x * kJxWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (slot >= last) return;
    const int64_t id = L.order[slot];
    const int64_t* tk = L.task + id * kJxTask;
    int64_t* row = L.out + id * kJxRow;
    const int64_t read = tk[0], xd = tk[3], yd = tk[4], xa = tk[5], ya = tk[6];
    const int minus = tk[1] != 0, want = (int)tk[7];
    const int status = jx_status(xd, yd, xa, ya, L.max_span);
    if (status != 0 || ya - yd > kJxClassBase * CPL) {             // the second cannot be: the host routes by jx_class, and such a row stays unwritten
        if (status != 0 && lane == 0) {
            row[0] = status;
#pragma unroll
            for (int f = 1; f < kJxRow; ++f) row[f] = 0;
        }
        return;
    }
    const int m = (int)(ya - yd);
    const int64_t coff = L.ctg_off[tk[2]], clen = L.ctg_len[tk[2]];
    const int nD = (int)jx_nd(xd, m, L.slack, clen), nA = (int)jx_na(xa, m, L.slack);
    const int8_t* rd = L.reads + L.read_off[read];
    const int64_t RL = L.read_off[read + 1] - L.read_off[read];

    int q[CPL], Lp[CPL], Lm[CPL], Rp[CPL], Rm[CPL], L0p, L0m, R0p, R0m;
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
        const int r = lane * CPL + k + 1;
        q[k] = r <= m ? jx_read_letter(rd, RL, yd + r - 1, minus) : 4;
    }
    jx_side<CPL>(L, lane, q, nD, coff, clen, xd, 1, xd, 0, Lp, Lm, L0p, L0m);
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
        const int r = lane * CPL + k + 1;
        q[k] = r <= m ? jx_read_letter(rd, RL, ya - r, minus) : 4;
    }
    jx_side<CPL>(L, lane, q, nA, coff, clen, xa - 1, -1, xa - 2, 1, Rp, Rm, R0p, R0m);

    // J of the lane's own rows t, the right side's row m - t fetched from the lane that holds it
    int64_t best = INT64_MIN;
#pragma unroll
    for (int k = CPL - 1; k >= 0; --k) {
        const int t = lane * CPL + k + 1, tp = m - t, kk = (m - k - 2) & (CPL - 1);
        const int rp = jx_row<CPL>(Rp, R0p, tp, kk), rm = jx_row<CPL>(Rm, R0m, tp, kk);
        if (t <= m) {
            const int64_t jp = (int64_t)(Lp[k] >> kJxIndexBits) + (rp >> kJxIndexBits) - L.io, jm = (int64_t)(Lm[k] >> kJxIndexBits) + (rm >> kJxIndexBits) - L.io;
            const int64_t cp = jp * 2048 + 1024 + (1023 - t), cm = jm * 2048 + (1023 - t);
            if (want >= 0 && cp > best) best = cp;
            if (want <= 0 && cm > best) best = cm;
        }
    }
    {                                                   // row 0, the same in every lane
        const int kk = (m - 1) & (CPL - 1);
        const int rp = jx_row<CPL>(Rp, R0p, m, kk), rm = jx_row<CPL>(Rm, R0m, m, kk);
        const int64_t jp = (int64_t)(L0p >> kJxIndexBits) + (rp >> kJxIndexBits) - L.io, jm = (int64_t)(L0m >> kJxIndexBits) + (rm >> kJxIndexBits) - L.io;
        const int64_t cp = jp * 2048 + 1024 + 1023, cm = jm * 2048 + 1023;
        if (want >= 0 && cp > best) best = cp;
        if (want <= 0 && cm > best) best = cm;
    }
    best = jx_wave_max(best);
    const int64_t J = best >> 11;                       // floor: the low 11 bits are the strand and 1023 - t
    const int sminus = (best & 1024) ? 0 : 1, t = 1023 - (int)(best & 1023);
    int Ls[CPL], Rs[CPL];
#pragma unroll
    for (int k = 0; k < CPL; ++k) { Ls[k] = sminus ? Lm[k] : Lp[k]; Rs[k] = sminus ? Rm[k] : Rp[k]; }
    const int lk = jx_row<CPL>(Ls, sminus ? L0m : L0p, t, (t - 1) & (CPL - 1));
    const int rk = jx_row<CPL>(Rs, sminus ? R0m : R0p, m - t, (m - t - 1) & (CPL - 1));
    if (lane == 0) {
        const int u = kJxIndexMask - (lk & kJxIndexMask), v = kJxIndexMask - (rk & kJxIndexMask);
        const int cs = jx_site(L.site, L.genome, coff, clen, xd + u, 0, sminus), ce = jx_site(L.site, L.genome, coff, clen, xa - v - 2, 1, sminus);
        row[0] = 0; row[1] = J; row[2] = sminus; row[3] = t; row[4] = u; row[5] = v; row[6] = xd + u; row[7] = xa - v;
        row[8] = (lk >> kJxIndexBits) + cs; row[9] = (rk >> kJxIndexBits) + ce; row[10] = cs; row[11] = ce;
    }
}

template <int C>
static hipError_t jx_launch_class(const JxLaunch& l, hipStream_t stream)
{
    const int64_t n = l.first[C + 1] - l.first[C];
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(seed_junction_kernel<(1 << C)>, dim3((unsigned)((n + kJxWaves - 1) / kJxWaves)), dim3(64 * kJxWaves), 0, stream, l, l.first[C], l.first[C + 1]);
    return hipGetLastError();
}

hipError_t launch_seed_junction(const JxLaunch& l, hipStream_t stream)
{
    static_assert(kJxClasses == 4 && kJxClassBase == 64, "one instantiation per class, a lane's first row in every class");
    hipError_t e = jx_launch_class<0>(l, stream);
    if (e == hipSuccess) e = jx_launch_class<1>(l, stream);
    if (e == hipSuccess) e = jx_launch_class<2>(l, stream);
    if (e == hipSuccess) e = jx_launch_class<3>(l, stream);
    return e;
}

__global__ void __launch_bounds__(256) genome_letters_kernel(const uint8_t* genome, int64_t genome_len, const int64_t* off, const int64_t* len, const int64_t* at,
                                                             int64_t n, int8_t* out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    for (int64_t k = 0; k < len[i]; ++k) out[at[i] + k] = (int8_t)jx_letter(genome, 0, genome_len, off[i] + k);
}

hipError_t launch_genome_letters(const uint8_t* genome, int64_t genome_len, const int64_t* off, const int64_t* len, const int64_t* at, int64_t n, int8_t* out,
                                 hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(genome_letters_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, genome, genome_len, off, len, at, n, out);
    return hipGetLastError();
}

}  // namespace clh
