// ssw_scan.hip -- K1s: Smith-Waterman scores and coordinates for SHORT reads, one alignment per wavefront (gfx950).
//
// Same answers as ssw_wavefront.hip (reference: libs/striped_smith_waterman/ssw.c:123-345 sw_sse2_byte and the
// forward + reverse orchestration of ssw_align, ssw.c:779-849; row-major statement: oracle/rowmajor_spec.c), for the
// alignments the host sorts into this class (clh_api.hip: scan_class_ok):
//     read <= 254 bases,  max_match * readLen + bias < 255  (ssw.c:804-806 then runs the 8-bit pass and that pass cannot
//     overflow: every score fits 8 bits, no 16-bit re-run, no stripe quirk),  gap_extend <= 16.
// These are the 20..300-base clips of find_bsj.py:191-216 against windows of 2 kb .. 400 kb -- most of the SSW calls of
// `call`.  The anti-diagonal kernel spends a fixed cost per step on handing three values down the lanes; with one row
// per virtual lane (reads <= 128 bases) that fixed cost is most of the step, and 127 fill/drain steps per pass are wasted.
//
// Here the matrix is walked the other way round: the lanes own reference columns, the loop runs over the read's rows
// (ssw_rowscan.h: the layout of a chunk, the row step, the prefix maximum that carries the gap along a row, the hand-over).
// What is this kernel's own:
//   * per column the running maximum over the rows is kept as (H << 8 | 255 - row): one unsigned maximum gives the
//     column maximum AND the smallest row that holds it (what ssw.c:299-308 searches at the end);
//   * the hand-over between chunks goes through 1 KiB of LDS;
//   * the reverse pass (ssw.c:834-849) ends at the first column whose maximum equals the forward score: it runs in chunks
//     of 256 columns and stops after the chunk that holds that column.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ssw_rowscan.h"

namespace clh {

namespace {

#ifndef SCAN_WAVES
#define SCAN_WAVES 3      // measured on the C3 clip batch: 2 -> 1.87 ms, 3 -> 1.76 ms, 4 -> 1.88 ms
#endif
static constexpr int SCAN_MAX_ROWS = 256;        // rows of a pass incl. the wildcard rows (reads <= 254 bases)

struct ScanIn : RsIn {    // terminate > 254 = never; colmax is indexed by col_base + column
    int own0;             // columns below this one are computed but do not count (the overlap of a window slice); 0 otherwise
    int col_base;         // column number of the first column handed in (a window slice); 0 otherwise
};
typedef RsOut ScanOut;

struct ScanLds {
    uint32_t* prof;       // RS_PROF_WORDS
    const int* mat;       // [6 reference codes][8 query codes]
    short* bH;            // [2][SCAN_MAX_ROWS]: H of the chunk's last column per row (parity of the chunk)
    short* bE;            // [2][SCAN_MAX_ROWS]: E entering the next chunk's first column per row
};

// one chunk of 128*CPR columns starting at column c0; returns through best_* the best cell so far (first column wins)
// and through tcol the first column of the chunk whose maximum equals in.terminate (or RS_INF)
template <int CPR, bool GEQ>
__device__ void scan_chunk(const ScanIn& in, const ScanLds& lds, const int c0, const int parity, const bool first, const bool more,
                           const int gapO, const int gapE, int& best_score, int& best_col, int& best_row, int& tcol)
{
    const int lane = threadIdx.x & 63;
    const int K = CPR * gapE;                    // what a gap loses across one virtual lane
    const int kLo = 2 * lane * K;
    const uint32_t gO2 = dup16(gapO), gE2 = dup16(gapE);

    rs_profile_fill<CPR, false>(in, lds.mat, lds.prof, c0);
    const RsHand hand(lds.bH, lds.bE, parity, SCAN_MAX_ROWS);
    __syncthreads();

    uint32_t Hp[CPR], Fst[GEQ ? 1 : CPR], key[CPR];
#pragma unroll
    for (int t = 0; t < CPR; ++t) { Hp[t] = 0; key[t] = 0; if constexpr (!GEQ) Fst[t] = 0; }
    int prev_hb = 0;                             // H[row - 1][c0 - 1]
    for (int rb = 0; rb < in.rows; rb += 64) {
        const int row = rb + lane;
        int qv = 5;
        if (row < in.L) qv = rs_read_code((int)in.read[(int64_t)row * in.rstep]);
        int hbv, ebv;
        hand.load(first, row, in.rows, hbv, ebv);
        const int cnt = in.rows - rb < 64 ? in.rows - rb : 64;
        int cobH = 0, cobE = 0;
        for (int i = 0; i < cnt; ++i) {
            const int q = __builtin_amdgcn_readlane(qv, i), hb = __builtin_amdgcn_readlane(hbv, i), eb = __builtin_amdgcn_readlane(ebv, i);
            uint32_t P[CPR], R[CPR];
            rs_profile_row<CPR>(lds.prof, q, lane, P);
            const uint32_t U = rs_row<CPR, GEQ>(Hp, prev_hb, Hp, Fst, P, gO2, gE2, R);
            const RsCarry cy = rs_lane_carry(U, eb, K, kLo);
            uint32_t Ein = cy.Ein;
            const uint32_t rowc = dup16(255 - (rb + i));
#pragma unroll
            for (int t = 0; t < CPR; ++t) {
                const uint32_t h = pk_max(R[t], Ein);
                Ein = pk_subs(Ein, gE2);
                Hp[t] = h;
                key[t] = pk_maxu(key[t], pk_madu(h, 0x01000100u, rowc));
            }
            prev_hb = hb;
            if (more) rs_handover_out(Hp[CPR - 1], cy, K, i, cobH, cobE);
        }
        hand.store(more, rb, cnt, cobH, cobE);
    }
    __syncthreads();

    // ---- the chunk's columns: column maxima out, terminate column, best cell (first column wins; smallest row in it) ----
    int tmin = RS_INF;
#pragma unroll
    for (int t = 0; t < CPR; ++t)
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            const int j = c0 + 2 * CPR * lane + hf * CPR + t;
            const int k16 = hf ? (int)(key[t] >> 16) : (int)(key[t] & 0xffffu);
            const int cm = k16 >> 8;
            if (j < in.ncols && j >= in.own0) {
                if (in.colmax) in.colmax[in.col_base + j] = (uint16_t)cm;
                if (cm == in.terminate) tmin = j < tmin ? j : tmin;
            }
        }
    tmin = wave_min(tmin);
    int b32 = 0;
#pragma unroll
    for (int t = 0; t < CPR; ++t)
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            const int jc = 2 * CPR * lane + hf * CPR + t, j = c0 + jc;
            const int k16 = hf ? (int)(key[t] >> 16) : (int)(key[t] & 0xffffu);
            const int v = ((k16 >> 8) << 20) | ((0xfff - jc) << 8) | (k16 & 0xff);
            if (j < in.ncols && j <= tmin && j >= in.own0) b32 = v > b32 ? v : b32;
        }
    b32 = wave_max(b32);
    const int sc = b32 >> 20;
    if (sc > best_score) { best_score = sc; best_col = c0 + (0xfff - ((b32 >> 8) & 0xfff)); best_row = 255 - (b32 & 0xff); }
    tcol = tmin;
}

template <bool GEQ>
__device__ ScanOut scan_pass(const ScanIn& in, const ScanLds& lds, const int gapO, const int gapE)
{
    int best_score = 0, best_col = -1, best_row = 0;
    const bool ends = in.terminate <= 254;       // reverse pass: stops at the first column whose maximum is the forward score
    int parity = 0;
    for (int c0 = 0; c0 < in.ncols; parity ^= 1) {
        const int rem = in.ncols - c0;
        int tcol = RS_INF;
        const bool first = c0 == 0;
        if (ends || rem <= 256) { scan_chunk<2, GEQ>(in, lds, c0, parity, first, rem > 256, gapO, gapE, best_score, best_col, best_row, tcol); c0 += 256; }
        else if (rem <= 512) { scan_chunk<4, GEQ>(in, lds, c0, parity, first, false, gapO, gapE, best_score, best_col, best_row, tcol); c0 += 512; }
        else { scan_chunk<8, GEQ>(in, lds, c0, parity, first, rem > 1024, gapO, gapE, best_score, best_col, best_row, tcol); c0 += 1024; }
        if (tcol != RS_INF) break;
    }
    ScanOut o;
    o.max = best_score;
    if (best_score == 0) { o.col = -1; o.row = 0; return o; }
    o.col = in.col_base + best_col;
    o.row = best_row < in.L - 1 ? best_row : in.L - 1;
    return o;
}

// everything after the forward pass: second best, reverse pass (begin coordinates), the result row
template <bool GEQ>
__device__ void scan_finish(const SswParams& p, const SswTask& task, const ScanOut& fw, const ScanLds& lds)
{
    const int lane = threadIdx.x & 63;
    const int8_t* read = p.reads + task.read_off;
    const int8_t* ref = p.refs + task.ref_off;
    const int refLen = task.ref_len;
    uint16_t* colmax = p.colmax ? p.colmax + task.colmax_off : nullptr;
    const int rdir = task.ref_rc ? -1 : 1;
    SswResult res;
    res.score2 = 0; res.ref_begin1 = -1; res.ref_end2 = 0; res.status = 0;
    res.score1 = fw.max;
    if (fw.max == 0) { res.ref_end1 = -1; res.read_end1 = 0; }
    else { res.ref_end1 = fw.col; res.read_end1 = fw.row; }
    if (task.mask_len >= 15 && colmax) { __syncthreads(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent"); second_best(colmax, refLen, res.ref_end1, task.mask_len, 0, res.score2, res.ref_end2); }
    else { res.score2 = 0; res.ref_end2 = task.mask_len >= 15 ? 0 : -1; }

    // ---- reverse: begin coordinates (ssw.c:834-849) ---------------------------------------------------------------
    res.read_begin1 = -1;
    const bool want_begin = !(p.flag == 0 || (p.flag == 2 && res.score1 < p.filters));
    if (want_begin) {
        ScanIn rv;
        rv.L = res.read_end1 + 1; rv.rows = ((rv.L + 15) / 16) * 16; rv.read = read + res.read_end1; rv.rstep = -1;
        rv.ncols = res.ref_end1 + 1; rv.ref = ref + (int64_t)res.ref_end1 * rdir; rv.cstep = -rdir; rv.comp = task.ref_rc;
        rv.terminate = res.score1; rv.colmax = nullptr; rv.own0 = 0; rv.col_base = 0;
        const ScanOut r = scan_pass<GEQ>(rv, lds, p.gapO, p.gapE);
        if (r.max == 0) { res.ref_begin1 = -1; res.read_begin1 = res.read_end1; }
        else { res.ref_begin1 = res.ref_end1 - r.col; res.read_begin1 = res.read_end1 - r.row; }
    }
    if (lane == 0) p.results[task.out_index] = res;
}

// the best of the slices' parts [first, first + count) of one alignment (first column on ties, ssw.c:283), and on as usual
template <bool GEQ>
__device__ void scan_finish_parts(const SswParams& p, const SswTask& task, const int first, const int count, const ScanLds& lds)
{
    int v = 0, c = RS_INF, r = 0;
    for (int k = threadIdx.x & 63; k < count; k += 64) {
        const ScanPart pt = p.parts[first + k];
        const int c2 = pt.max > 0 ? pt.col : RS_INF;
        const bool take = pt.max > v || (pt.max == v && c2 < c);
        v = take ? pt.max : v; c = take ? c2 : c; r = take ? pt.row : r;
    }
    rs_best_of(v, c, r);        // (slices own different columns: the end row only travels along)
    ScanOut fw; fw.max = v; fw.col = v > 0 ? c : -1; fw.row = v > 0 ? r : 0;
    scan_finish<GEQ>(p, task, fw, lds);
}

// forward pass over columns [c_begin, c_end) of the task's window, counting from own_begin on (ssw.c:804-822: the 8-bit
// pass; it cannot overflow in this class)
template <bool GEQ>
__device__ ScanOut scan_forward(const SswParams& p, const SswTask& task, const ScanLds& lds, int c_begin, int own_begin, int c_end)
{
    const int rdir = task.ref_rc ? -1 : 1;
    uint16_t* colmax = p.colmax ? p.colmax + task.colmax_off : nullptr;
    ScanIn in;
    in.read = p.reads + task.read_off; in.rstep = 1; in.L = task.read_len;
    in.ref = p.refs + task.ref_off + (int64_t)c_begin * rdir; in.cstep = rdir; in.comp = task.ref_rc; in.ncols = c_end - c_begin;
    in.terminate = 1 << 30; in.colmax = colmax; in.own0 = own_begin - c_begin; in.col_base = c_begin;
    in.rows = colmax ? ((in.L + 15) / 16) * 16 : in.L;     // the wildcard rows only matter to the column maxima (rowmajor_spec.c)
    return scan_pass<GEQ>(in, lds, p.gapO, p.gapE);
}
__device__ __forceinline__ ScanPart scan_part(const ScanOut& fw) { ScanPart pt; pt.max = fw.max; pt.col = fw.col; pt.row = fw.row; pt.pad = 0; return pt; }

#define SCAN_LDS_SETUP \
    __shared__ __attribute__((aligned(16))) uint32_t s_prof[RS_PROF_WORDS]; \
    __shared__ int s_mat[48]; \
    __shared__ short s_bH[2 * SCAN_MAX_ROWS], s_bE[2 * SCAN_MAX_ROWS]; \
    ScanLds lds; lds.prof = s_prof; lds.mat = s_mat; lds.bH = s_bH; lds.bE = s_bE; \
    rs_stage_matrix(p.mat, p.n, s_mat);

}  // namespace

template <bool GEQ>
__global__ void __launch_bounds__(64, SCAN_WAVES) ssw_scan_kernel(const SswParams p)
{
    SCAN_LDS_SETUP
    const SswTask task = p.tasks[blockIdx.x];
    const ScanOut fw = scan_forward<GEQ>(p, task, lds, 0, 0, task.ref_len);
    scan_finish<GEQ>(p, task, fw, lds);
}

// Long windows (clh_api.hip: scan_slices): the forward pass of one alignment is cut into slices of the window that run as
// separate workgroups (ssw_rowscan.h, rs_static_slices: why a slice started `overlap` columns early is exact).  Each slice
// leaves its best cell; the finishing kernel takes the largest (first column on ties, ssw.c:283) and goes on as usual.
template <bool GEQ>
__global__ void __launch_bounds__(64, SCAN_WAVES) ssw_scan_slice_kernel(const SswParams p)
{
    SCAN_LDS_SETUP
    const ScanSlice sl = p.slices[blockIdx.x];
    const SswTask task = p.tasks[sl.task];
    const ScanOut fw = scan_forward<GEQ>(p, task, lds, sl.c_begin, sl.own_begin, sl.c_end);
    if ((threadIdx.x & 63) == 0) p.parts[sl.part] = scan_part(fw);
}

template <bool GEQ>
__global__ void __launch_bounds__(64, SCAN_WAVES) ssw_scan_finish_kernel(const SswParams p)
{
    SCAN_LDS_SETUP
    const SswTask task = p.tasks[blockIdx.x];
    scan_finish_parts<GEQ>(p, task, (int)task.dir_off, task.pad, lds);       // this task's slices (clh_api.hip: at most 64)
}

// What the pick kernels share: with the seed's score S0 in hand, the candidate blocks of the alignment (ssw_rowscan.h, rs_pick_count), their
// runs as slices in the queue -- or the static slices when the runs outnumber the alignment's share of the queue or cover about as much as
// the window -- and the alignment's PfOut.  stage2_ok: the caller may still send the window to the second stage; returns true when it
// should (the candidates cover more than an eighth of the window: the indel-distance pass over the window costs about as much as the
// score pass over a twelfth of it; and the threshold is below what that distance is on random text) and then writes nothing.
template <bool GEQ>
__device__ bool pf_pick_emit(const SswParams& p, const SswTask& task, const PfWin& pt, const uint8_t* dmin, const int S0, const ScanOut& seed, const int seed_block,
                             const bool stage2_ok)
{
    const int R = task.ref_len, L = task.read_len;
    const RsSlices ss = rs_static_slices<false>(p, R, L);
    RsPick pk; pk.ov_c = ss.overlap;
    if (dmin && S0 > 0) {
        pk = rs_pick_count(p, dmin, pt.nsub, R, L, S0, ss, pt.nsub / 8 + 1 > 64 ? pt.nsub / 8 + 1 : 64);
        // (the indel distance of a clip to random text is ~0.58 L, less for short clips: above 0.55 L the second stage cannot help either)
        if (stage2_ok && (p.pf2_always || ((!pk.pruned || pk.cost > (long long)R / p.pf2_share) && 20 * pk.thr < 11 * L))) return true;
    }
    const int count = pk.pruned ? pk.nrun : ss.nstatic;
    const int first = rs_pick_reserve(p, count, pk.pruned, R);
    unsigned long long cols = 0;
    // slice k of the alignment owns [b0, b1) and starts ov columns early; seeded: its best cell is known already (the seed's own region)
    auto emit = [&](const int k, const int b0, const int b1, const int ov, const bool seeded) {
        ScanSlice sl;
        sl.task = seeded ? -1 : (int)blockIdx.x; sl.own_begin = b0; sl.c_begin = b0 - ov < 0 ? 0 : b0 - ov; sl.c_end = b1;
        sl.part = first + k; sl.pad0 = sl.pad1 = sl.pad2 = 0;
        if (seeded) p.parts[sl.part] = scan_part(seed); else cols += (unsigned long long)(b1 - sl.c_begin);
        p.pf_slices[sl.part] = sl;
    };
    if (pk.pruned) rs_for_each_run(dmin, pt.nsub, pk.thr, pt.phase, R, [&](int rank, int b0, int b1, int len, int k) { emit(rank, b0, b1, pk.ov_c, len == 1 && k == seed_block); });
    else rs_for_each_static(ss, R, [&](int k, int b0, int b1) { emit(k, b0, b1, ss.overlap, false); });
    PfOut o; o.first = first; o.count = count; o.s0 = S0; o.pruned = pk.pruned;
    rs_pick_close(p, cols, o);
    return false;
}

// ---- the sliced class behind the prefilter (ssw_prefilter.hip; tools/prefilter_model.py) --------------------------------------
// One wave per task: (1) the block with the smallest minimum of d; a forward pass around it ATTAINS a score S0; (2) every
// block whose minimum is at most (M L - S0) / c is a candidate -- no other block can hold the maximum or tie it; runs of
// candidate blocks (cut at groups of 64) become slices in the queue, each started `overlap` columns early like a static slice;
// (3) when the runs outnumber the task's share of the queue or cover about as much as the window, the static slices of
// clh_api.hip are written instead -- or, with a second stage (p.pf_q2), the window's entries of the work list are queued for the
// indel-distance pass and ssw_scan_pick2_kernel decides.  p.pf_dmin == nullptr (filter off for this run): static slices at once.
template <bool GEQ>
__global__ void __launch_bounds__(64, SCAN_WAVES) ssw_scan_pick_kernel(const SswParams p)
{
    SCAN_LDS_SETUP
    const int lane = threadIdx.x & 63;
    const SswTask task = p.tasks[blockIdx.x];
    const PfWin pt = p.pf_win[blockIdx.x];
    const int R = task.ref_len;
    const uint8_t* dmin = p.pf_dmin ? p.pf_dmin + p.pf_tasks[pt.piece_first].sub_off : nullptr;     // (one piece: reads of this class have <= 254 bases)
    int S0 = 0, seed_block = -1;
    ScanOut seed; seed.max = 0; seed.col = -1; seed.row = 0;
    if (dmin) {
        int key = RS_INF;
        for (int k = lane; k < pt.nsub; k += 64) { const int v = ((int)dmin[k] << 20) | k; key = v < key ? v : key; }
        key = wave_min(key);
        const int kb = key & 0xfffff;
        int c0 = kb * kPfBlock - pt.phase, c1 = c0 + kPfBlock;
        c0 = c0 < 0 ? 0 : c0; c1 = c1 > R ? R : c1;
        const int overlap = rs_static_slices<false>(p, R, task.read_len).overlap;
        seed = scan_forward<GEQ>(p, task, lds, c0 - overlap < 0 ? 0 : c0 - overlap, c0, c1);
        S0 = seed.max; seed_block = kb;
    }
    if (pf_pick_emit<GEQ>(p, task, pt, dmin, S0, seed, seed_block, p.pf_q2 != nullptr && dmin != nullptr)) {
        // the unit-cost bound leaves too much of this window: its entries of the work list once more, with the indel distance
        int base = 0;
        if (lane == 0) {
            base = atomicAdd(&p.pf_ctl->q2count, pt.work_count);
            atomicAdd(&p.pf_ctl->n_stage2, 1);
            PfOut o; o.first = 0; o.count = 0; o.s0 = S0; o.pruned = 2;          // 2: pending (ssw_scan_pick2_kernel)
            p.pf_out[blockIdx.x] = o;
        }
        base = __builtin_amdgcn_readfirstlane(base);
        for (int k = lane; k < pt.work_count; k += 64) p.pf_q2[base + k] = pt.work_first + k;
    }
}

// after the second stage: the windows it took (PfOut.pruned == 2), by its block minima
template <bool GEQ>
__global__ void __launch_bounds__(64, SCAN_WAVES) ssw_scan_pick2_kernel(const SswParams p)
{
    const PfOut po = p.pf_out[blockIdx.x];
    if (po.pruned != 2) return;
    const SswTask task = p.tasks[blockIdx.x];
    const PfWin pt = p.pf_win[blockIdx.x];
    const uint8_t* dmin = p.pf_dmin + p.pf_tasks[pt.piece_first].sub_off;
    ScanOut seed; seed.max = 0; seed.col = -1; seed.row = 0;
    (void)pf_pick_emit<GEQ>(p, task, pt, dmin, po.s0, seed, -1, false);
}

// the queue's slices by persistent workgroups (the number of slices is only known on the device)
template <bool GEQ>
__global__ void __launch_bounds__(64, SCAN_WAVES) ssw_scan_queue_kernel(const SswParams p)
{
    SCAN_LDS_SETUP
    const int total = p.pf_ctl->qcount;
    for (int idx; (idx = rs_next(&p.pf_ctl->qnext)) < total;) {
        const ScanSlice sl = p.pf_slices[idx];
        if (sl.task < 0) continue;                 // the seed's region: done by the pick kernel
        const SswTask task = p.tasks[sl.task];
        const ScanOut fw = scan_forward<GEQ>(p, task, lds, sl.c_begin, sl.own_begin, sl.c_end);
        if ((threadIdx.x & 63) == 0) p.parts[sl.part] = scan_part(fw);
        __syncthreads();
    }
}

template <bool GEQ>
__global__ void __launch_bounds__(64, SCAN_WAVES) ssw_scan_finish_queue_kernel(const SswParams p)
{
    SCAN_LDS_SETUP
    const PfOut po = p.pf_out[blockIdx.x];
    scan_finish_parts<GEQ>(p, p.tasks[blockIdx.x], po.first, po.count, lds);
}

hipError_t launch_ssw_scan_filtered(bool geq, const SswParams& p, int ntasks, int nworkgroups, int nworkgroups2, hipStream_t stream)
{
    const bool stage2 = p.pf_q2 != nullptr && p.pf_dmin != nullptr;
    return with_geq(geq, [&](auto g) {
        constexpr bool G = decltype(g)::value;
        hipLaunchKernelGGL((ssw_scan_pick_kernel<G>), dim3(ntasks), dim3(64), 0, stream, p);
        if (stage2) {
            if (hipError_t e = launch_ssw_prefilter_indel(p, nworkgroups2, stream)) return e;
            hipLaunchKernelGGL((ssw_scan_pick2_kernel<G>), dim3(ntasks), dim3(64), 0, stream, p);
        }
        hipLaunchKernelGGL((ssw_scan_queue_kernel<G>), dim3(nworkgroups), dim3(64), 0, stream, p);
        hipLaunchKernelGGL((ssw_scan_finish_queue_kernel<G>), dim3(ntasks), dim3(64), 0, stream, p);
        return hipGetLastError();
    });
}

hipError_t launch_ssw_scan(bool geq, const SswParams& p, int ntasks, hipStream_t stream)
{
    return with_geq(geq, [&](auto g) {
        hipLaunchKernelGGL((ssw_scan_kernel<decltype(g)::value>), dim3(ntasks), dim3(64), 0, stream, p);
        return hipGetLastError();
    });
}

// class kRvCombine: the best of an alignment's window-slice tasks (clh_api.hip) becomes its result row: largest score, then
// smallest end column in the whole window, then the earlier slice (the one that owns that column)
__global__ void __launch_bounds__(64) ssw_combine_kernel(const SswParams p)
{
    const int lane = threadIdx.x & 63;
    const SswTask task = p.tasks[blockIdx.x];
    const int first = (int)task.dir_off, ns = task.pad;
    int v = -1, c = RS_INF, k = RS_INF;
    if (lane < ns) {
        const SswResult r = p.results[p.n_real + first + lane];
        v = r.score1; k = lane;
        c = r.score1 > 0 ? r.ref_end1 + p.slice_base[first + lane] : RS_INF;
    }
    rs_best_of(v, c, k);
    if (lane == 0) {
        SswResult r = p.results[p.n_real + first + k];
        rs_shift_row(r, p.slice_base[first + k]);
        p.results[task.out_index] = r;
    }
}

hipError_t launch_ssw_combine(const SswParams& p, int ntasks, hipStream_t stream)
{
    hipLaunchKernelGGL(ssw_combine_kernel, dim3(ntasks), dim3(64), 0, stream, p);
    return hipGetLastError();
}

// p.slices / p.parts set; p.tasks = the sliced class's tasks
hipError_t launch_ssw_scan_sliced(bool geq, const SswParams& p, int ntasks, int nslices, hipStream_t stream)
{
    return with_geq(geq, [&](auto g) {
        constexpr bool G = decltype(g)::value;
        hipLaunchKernelGGL((ssw_scan_slice_kernel<G>), dim3(nslices), dim3(64), 0, stream, p);
        hipLaunchKernelGGL((ssw_scan_finish_kernel<G>), dim3(ntasks), dim3(64), 0, stream, p);
        return hipGetLastError();
    });
}

}  // namespace clh
