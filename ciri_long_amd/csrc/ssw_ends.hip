// ssw_ends.hip -- K1g: end-anchored affine-gap alignment of pairs (global, semiglobal, overlap; start-anchored: prefix, extend) in
// int32 cells, under one-piece, two-piece and intron gap costs (gfx950).
//
// The frame, the same for every gap model.  The row-scan form of K1w (ssw_scan_wide.hip) without its packing: one wave takes one
// pair, its 64 lanes own kEnCpl consecutive reference columns each (a chunk of kEnChunk columns), the loop runs over the query rows,
// and a longer reference is walked chunk after chunk, a chunk handing what the next needs of its last column on, NH values per row
// (two buffers, written by one chunk and read by the next).  E along the row is a max-plus prefix scan over the lanes
// (wave_prefix_max + one DPP move), F is lane-private.  No cell holds minus infinity: F of row 0 and E of column 0 enter as H - go,
// which gives the same first F and E, so every value is the score of an alignment (or one gap opening below it) and the host's bound
// (m + n) max(|s|, every gap cost) < 2^30 keeps int32.
// The mode is a template parameter: the boundary values, and which end cells are followed (the last row's running maximum keyed
// by the smallest column, the last column's keyed by the smallest row in the lane that owns column n, the corner).
// prefix and extend have global's boundary.  prefix ends where semiglobal does, the last row's maximum seeded with H[m][0].  extend
// ends at the greatest H of all cells, smallest i, then smallest j, (0, 0) with 0 included: every lane keeps the best (value, i, k)
// of its own cells of a chunk under a bare > (rows ascend, columns ascend within a row: the first is the smallest key), joins it
// to the best it carries over the chunks by the key (a later chunk's columns are larger, its rows may be smaller), and the lanes
// are reduced once, after the last chunk.  Boundary cells but (0, 0) are <= 0 and lose every tie to (0, 0), the seed of every lane.
// STORE: each cell also leaves its decisions, one word per lane and row, and ssw_ends_walk_kernel<Prm> walks them back, one lane per
// pair (as K4t does): the walk (pr_walk<MODEL>) and where the word of a cell lies (EnCells) are in ssw_pairs.h, the walk shared with K1gb.
// The gap model is a constant derived from the parameter block, and ssw_ends_kernel is one body for the three: the frame above is
// written once, and what a model has of its own (boundary values, the per-chunk set-up, the incoming column, the row step, the
// decision word, what is handed on) stands under `if constexpr`, so that an instantiation holds its model's statements and no other.
// No device helper stands in or around the row loop: as helpers, the epilogue and the end-cell tracking changed the storing forms'
// register allocation or put scratch into them (LABNOTES.md 16 and 20).
//
// One piece (EnParams): a gap of k letters costs go + (k - 1) ge.  Per row step and lane:
//     F[k] = max(Hprev[k] - go, Fprev[k] - ge)                        lane-private
//     T[k] = max(diag[k] + s, F[k])                                   H without E
//     V    = max over k of T[k] - go + (p + 1) ge                     p = 8 lane + k, the column inside the chunk
//     u    = exclusive prefix maximum of V over the lanes (wave_prefix_max + one DPP move), lane 0 seeded with E of column 0
//     E[k] = u - p ge,  H[k] = max(T[k], E[k]),  u = max(u, T[k] - go + (p + 1) ge)
// -- E[j] = max(E[j-1] - ge, H[j-1] - go) as a max-plus scan in the frame E[p] + p ge, exact because go >= ge lets T stand for H.
// A chunk hands H and E of its last column on.  STORE: 4 bits per cell -- H's source (0 diagonal, 1 E, 2 F; that order is the tie
// rule), "E opened here", "F opened here" -- one 32-bit word per lane and row.
// tools/ends_model.py is this scheme in Python for any geometry; tests/ends_check.py is the definition.
//
// Two pieces (En2Params): a gap of k letters costs min(go + (k - 1) ge, go2 + (k - 1) ge2); go / ge / E / F are piece 1 below and
// go2 / ge2 / E2 / F2 piece 2.  Per row step and lane:
//     F_p[k] = max(Hprev[k] - go_p, F_pprev[k] - ge_p)                p = 1, 2, lane-private
//     T[k]   = max(diag[k] + s, F_1[k], F_2[k])                       H without E
//     V_p    = max over k of T[k] - go_p + (c + 1) ge_p               c = 8 lane + k; two scans, each in its own frame E_p + c ge_p
//     u_p    = exclusive prefix maximum of V_p over the lanes, lane 0 seeded with E_p of the chunk's column 0; the two
//              wave_prefix_max chains are independent and the compiler interleaves them
//     e_p    = u_p - (8 lane) ge_p,  then along the lane  E_p[k] = e_p,  H[k] = max(T[k], E_1[k], E_2[k]),
//              e_p = max(e_p - ge_p, T[k] - go_p)
// The scan of piece p sees T - go_p and E_p - ge_p, not the definition's H - go_p: H may be the other piece's E.  Under the
// admitted costs 0 <= ge2 <= ge1 <= go1 <= go2 that cross term never reaches H and never changes a value the walk reads:
//     E_2[j'] - go1 - k ge1 <= E_2[j'] - (k + 1) ge2 <= E_2[j' + k + 1], and a piece-1 run of a + 1 letters followed by a piece-2 opening
//     costs go1 + a ge1 + go2 + k ge2 >= go2 + (a + 1 + k) ge2, the one piece-2 run from the same start;
//     equality in either needs go1 == ge2, hence ge2 == ge1 == go1: then piece 2 is dominated, E_2 <= E_1 in every cell, and the
//     term is inside E_1's own scan.
// F_p reads the true H of the row above.  A chunk hands H, E_1 and E_2 of its last column on: three values per row.
// STORE: one byte per cell -- bits 0..2 H's source (0 diagonal, 1 E_1, 2 E_2, 3 F_1, 4 F_2; that order is the tie rule), bit 3
// "E_1 opened here", bit 4 "E_2 opened here", bit 5 "F_1 opened here", bit 6 "F_2 opened here" -- 8 bytes per lane and row, one
// 8-byte store; the walk loads them a byte at a time.  tests/twopiece_check.py is the definition.
//
// Intron gaps (SpParams): a maximal run of skipped reference letters r[a..b] costs min(go + (b - a) ge, io + start(a) + end(b)), the
// splice-site costs start / end read from the dinucleotides at the run's two ends on the pair's strand.  With don(j) = start(j - 1)
// and acc(j) = end(j - 1) for the 1-based column j, per row step and lane:
//     F[k] = max(Hprev[k] - go, Fprev[k] - ge)                        lane-private; reads the true H
//     T[k] = max(diag[k] + s, F[k])                                   H without a reference gap
//     V    = max over k of T[k] - go + (p + 1) ge                     p = 8 lane + k; the max-plus scan of E as under two pieces
//     W    = max over k of T[k] - io - don(j + 1)                     the intron costs nothing per letter: a plain prefix maximum
//     e, u = exclusive prefix maxima of V and W over the lanes, lane 0 seeded with E and N of the chunk's first column
//     along the lane  E[k] = e,  N[k] = u,  H[k] = max(T[k], E[k], N[k] - acc(j)),  e = max(e - ge, T[k] - go),  u = max(u, T[k] - io - don(j + 1))
// E and N open from T, never from H: a deletion run and an intron run are never adjacent, which is what makes the one rule exact
// (tests/spliced_check.py is the definition).  io + don(j + 1) and acc(j) depend on the column alone and are set up once per chunk from
// the lane's own letters, one letter before and two after them; a dinucleotide with a code >= 4 or a letter off the reference costs
// `other`.  Both strands' tables lie in LDS (in these instantiations alone) as costs of the dinucleotide as the reference reads it (the
// host complements them for strand -).  A chunk hands T, E and N of its last column on, three values per row; the next chunk rebuilds
// that column's H = max(T, E, N - acc) for its first diagonal.  (H in place of T would let a deletion follow an intron, or an intron a
// deletion, across the chunk edge.)  Row 0 of the anchored modes is H[0][j] = -min(go + (j - 1) ge, io + don(1) + acc(j)).  E and N of
// column 0 enter as one opening below T, which gives the same first E and N; the host's bound takes io + dmax + amax among the costs.
// STORE: one byte per cell -- bits 0..1 H's source (0 diagonal, 1 E, 2 N, 3 F; that order is the tie rule), bit 2 T's source (0
// diagonal, 1 F), bit 3 "E opened here", bit 4 "N opened here", bit 5 "F opened here" -- 8 bytes per lane and row, one 8-byte store;
// the walk holds the 8 bytes it loaded last and takes an E or N run up to 8 cells a step out of them.  tools/spliced_model.py is this scheme in Python.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "clh_device.h"
#include "clh_device_ops.h"
#include "ssw_pairs.h"

namespace clh {

static_assert(kEnCpl == 8, "a lane's row of decisions is one 32-bit word (8 columns x 4 bits) or two (8 columns x 1 byte)");

// the gap model of a parameter block: NH values per row are handed from chunk to chunk, a lane's row of decisions is one word_t, and
// the walk loads a cell_t at a time (EnCells in ssw_pairs.h)
template <typename Prm> struct EnModel;
template <> struct EnModel<EnParams> { static constexpr int model = EN_ONE_PIECE, NH = 2; typedef uint32_t word_t; typedef uint32_t cell_t; };
template <> struct EnModel<En2Params> { static constexpr int model = EN_TWO_PIECE, NH = 3; typedef uint2 word_t; typedef uint8_t cell_t; };
template <> struct EnModel<SpParams> { static constexpr int model = EN_SPLICED, NH = 3; typedef uint2 word_t; typedef uint2 cell_t; };

// H[0][j]: 0 on a free row, one gap of j letters in the global mode (unsigned arithmetic: lanes past column n hold garbage, not UB)
template <int MODE>
__device__ __forceinline__ int en_row0(int j, int go, int ge)
{
    return (en_anchored(MODE) && j > 0) ? (int)(0u - (uint32_t)go - (uint32_t)(j - 1) * (uint32_t)ge) : 0;
}
template <int MODE>
__device__ __forceinline__ int en_col0(int i, int go, int ge)
{
    return (MODE == EN_OVERLAP || i == 0) ? 0 : (int)(0u - (uint32_t)go - (uint32_t)(i - 1) * (uint32_t)ge);
}

// two pieces: minus the cost of one gap of j letters, j >= 1 (unsigned arithmetic: lanes past column n hold garbage, not UB)
__device__ __forceinline__ int en2_gap(int j, const En2Params& prm)
{
    const int a = (int)(0u - (uint32_t)prm.go - (uint32_t)(j - 1) * (uint32_t)prm.ge);
    const int b = (int)(0u - (uint32_t)prm.go2 - (uint32_t)(j - 1) * (uint32_t)prm.ge2);
    return pr_max(a, b);
}
template <int MODE>
__device__ __forceinline__ int en2_row0(int j, const En2Params& prm) { return (en_anchored(MODE) && j > 0) ? en2_gap(j, prm) : 0; }
template <int MODE>
__device__ __forceinline__ int en2_col0(int i, const En2Params& prm) { return (MODE == EN_OVERLAP || i == 0) ? 0 : en2_gap(i, prm); }

// spliced: the cost of the dinucleotide (x, y) as the reference reads it; site[0..15] start and site[16..31] end of the strand, site[kSpOther] other
__device__ __forceinline__ int sp_site(const int* site, int strand_off, int which, int x, int y)
{
    return site[((x | y) > 3) ? kSpOther : strand_off + which + 4 * x + y];
}
// spliced: H[0][j], j >= 1: 0 on a free row, else the cheaper of one deletion and one intron of j letters; iod1 = io + don(1), a = acc(j)
template <int MODE>
__device__ __forceinline__ int sp_row0(int j, int go, int ge, int iod1, int a)
{
    if (!en_anchored(MODE)) return 0;
    const int del = (int)((uint32_t)go + (uint32_t)(j - 1) * (uint32_t)ge), intron = iod1 + a;
    return -(del < intron ? del : intron);
}

// FORM: the score pass alone; the storing form; and the two passes of the recompute route -- the keeping form, the score pass with
// every chunk's hand-over kept in a slot of its own (slot c written by chunk c, read by chunk c + 1) in the pair's block of the
// workspace, which also leaves the walk's fresh resume record; and the tile form, the storing row step over the one chunk and the
// rows 1..i that the record names, its incoming column from kept slot c - 1, its words in the block's one-chunk plane (EnTile).
enum { EN_SCORE = 0, EN_STORE = 1, EN_KEEP = 2, EN_TILE = 3 };
template <typename Prm, int MODE, int FORM>
__global__ void __launch_bounds__(64) ssw_ends_kernel(const Prm prm, int first, int count)
{
    constexpr bool STORE = FORM == EN_STORE || FORM == EN_TILE, KEPT = FORM == EN_KEEP || FORM == EN_TILE;
    constexpr int model = EnModel<Prm>::model, NH = EnModel<Prm>::NH;
    typedef typename EnModel<Prm>::word_t word_t;
    __shared__ int smat[32 * 32];                    // [query code][reference code]
    __shared__ int site[model == EN_SPLICED ? kSpSites : 1];             // spliced alone reads or writes it
    const int lane = threadIdx.x & 63;
    if constexpr (model == EN_SPLICED)
        for (int k = lane; k < kSpSites; k += 64) site[k] = prm.site[k];
    pr_load_matrix(smat, prm.mat, prm.n_mat, lane);  // ends on the barrier that also publishes `site`
    const int x = (int)blockIdx.x;
    if (x >= count || first + x >= prm.npairs) return;
    const EnPair pr = prm.pairs[first + x];
    const int m = pr.m, n = pr.n;
    if (m <= 0 || n <= 0) return;                    // an empty side is answered by fetch
    const int go = prm.go, ge = prm.ge;
    int go2 = 0, ge2 = 0, io = 0, soff = 0;          // two pieces: piece 2; spliced: the intron's opening and the strand's half of `site`
    if constexpr (model == EN_TWO_PIECE) { go2 = prm.go2; ge2 = prm.ge2; }
    if constexpr (model == EN_SPLICED) { io = prm.io; soff = (prm.strand && prm.strand[first + x] < 0) ? 32 : 0; }
    const int nchunks = (n + kEnChunk - 1) / kEnChunk;
    const int mpad = (m + 63) & ~63;
    // hand-over buffers of this pair: [buffer 0 / 1][H, E / H, E_1, E_2 / T, E, N][mpad]
    int32_t* hand;
    int32_t* rec = nullptr;                          // kept forms: the walk's resume record
    word_t* tile = nullptr;                          // tile form: the one-chunk plane
    int tc = 0, ti = 0;                              // tile form: the chunk and the row limit
    if constexpr (!KEPT) {
        if (nchunks > 1 && (pr.hand_off < 0 || pr.hand_off + (int64_t)(2 * NH) * mpad > prm.hand_cap)) return;
        hand = prm.hand + (nchunks > 1 ? pr.hand_off : 0);
    } else {
        const EnKept lay(m, n, NH, (int)sizeof(word_t));
        if (!lay.fits(pr.ws_off, prm.ws_cap)) return;            // the keeping form leaves the row unwritten, and every later pass returns here too
        hand = (int32_t*)(prm.ws + pr.ws_off);
        rec = (int32_t*)(prm.ws + pr.ws_off + lay.rec_off);
        if constexpr (FORM == EN_TILE) {
            if (prm.rows[(size_t)(first + x) * 8 + 7] != 0 || rec[EN_REC_DONE] != 0 || rec[EN_REC_J] <= 0) return;
            tile = (word_t*)(prm.ws + pr.ws_off + lay.plane_off);
            tc = rec[EN_REC_CHUNK]; ti = rec[EN_REC_I];
            tc = tc < 0 ? 0 : (tc > nchunks - 1 ? nchunks - 1 : tc);
            ti = ti > m ? m : ti;
            if (ti <= 0) return;
        }
    }
    const int mr = FORM == EN_TILE ? ti : m;         // the rows of the pass
    const int8_t* qry = prm.qry + pr.q_off;
    const int8_t* ref = prm.ref + pr.r_off;
    auto letter = [&](int pos) -> int { return (pos >= 0 && pos < n) ? ((int)ref[pos] & 31) : 4; };      // spliced; 0-based; 4 off the reference
    bool ws_ok = true;
    if (FORM == EN_STORE) {
        const int llast = (n - (nchunks - 1) * kEnChunk + kEnCpl - 1) / kEnCpl;
        const int64_t need = (int64_t)sizeof(word_t) * m * ((int64_t)64 * (nchunks - 1) + llast);
        ws_ok = pr.ws_off >= 0 && (pr.ws_off & (int64_t)(sizeof(word_t) - 1)) == 0 && pr.ws_off + need <= prm.ws_cap;
    }

    int row_best, row_j = 0;                                   // the last row's running maximum, smallest column
    if constexpr (model == EN_TWO_PIECE) row_best = en2_col0<MODE>(m, prm);
    else row_best = en_col0<MODE>(m, go, ge);
    int col_best = 0, col_i = 0, corner = 0;                   // the last column's (H[0][n] = 0 where it counts), smallest row; H[m][n]
    const int ln = ((n - 1) % kEnChunk) / kEnCpl, kn = ((n - 1) % kEnChunk) % kEnCpl;
    int ext_v = 0, ext_i = 0, ext_j = 0;                       // extend: the best cell this lane has seen, seeded with (0, 0)
    int base = 0, base2 = 0, iod1 = 0;                         // two pieces and spliced: the lane's place in a scan's frame; spliced: io + don(1)
    if constexpr (model == EN_TWO_PIECE) { base = (int)((uint32_t)(lane * kEnCpl) * (uint32_t)ge); base2 = (int)((uint32_t)(lane * kEnCpl) * (uint32_t)ge2); }
    if constexpr (model == EN_SPLICED) {
        base = (int)((uint32_t)(lane * kEnCpl) * (uint32_t)ge);
        iod1 = io + sp_site(site, soff, 0, letter(0), letter(1));
    }

    for (int c = FORM == EN_TILE ? tc : 0; c < (FORM == EN_TILE ? tc + 1 : nchunks); ++c) {
        const int c0 = c * kEnChunk;
        const bool last = c == nchunks - 1;
        const int cols = last ? n - c0 : kEnChunk;
        const int L = (cols + kEnCpl - 1) / kEnCpl;            // lanes with a column
        int rcode[kEnCpl], off[kEnCpl], Hp[kEnCpl], Fp[kEnCpl], hleft;     // hleft: H[i-1][first own column - 1]
        int poff[kEnCpl];                                      // one piece
        int off2[kEnCpl], F2p[kEnCpl];                         // two pieces
        int iod[kEnCpl], acc[kEnCpl], iod_in = 0, acc_in = 0;  // spliced
        if constexpr (model == EN_ONE_PIECE) {
#pragma unroll
            for (int k = 0; k < kEnCpl; ++k) {
                const int p = lane * kEnCpl + k, j = c0 + 1 + p;
                rcode[k] = j <= n ? ((int)ref[j - 1] & 31) : 0;
                poff[k] = (int)((uint32_t)p * (uint32_t)ge);
                off[k] = (int)((uint32_t)(p + 1) * (uint32_t)ge - (uint32_t)go);
                Hp[k] = en_row0<MODE>(j, go, ge);
                Fp[k] = Hp[k] - go;
            }
            hleft = en_row0<MODE>(c0 + lane * kEnCpl, go, ge);
        } else if constexpr (model == EN_TWO_PIECE) {
#pragma unroll
            for (int k = 0; k < kEnCpl; ++k) {
                const int p = lane * kEnCpl + k, j = c0 + 1 + p;
                rcode[k] = j <= n ? ((int)ref[j - 1] & 31) : 0;
                off[k] = (int)((uint32_t)(p + 1) * (uint32_t)ge - (uint32_t)go);
                off2[k] = (int)((uint32_t)(p + 1) * (uint32_t)ge2 - (uint32_t)go2);
                Hp[k] = en2_row0<MODE>(j, prm);
                Fp[k] = Hp[k] - go;
                F2p[k] = Hp[k] - go2;
            }
            hleft = en2_row0<MODE>(c0 + lane * kEnCpl, prm);
        } else {
            // what the column in front of the chunk needs: io + don(c0 + 1), acc(c0) and H[0][c0]
            iod_in = io + sp_site(site, soff, 0, letter(c0), letter(c0 + 1));
            acc_in = sp_site(site, soff, 16, letter(c0 - 2), letter(c0 - 1));
            const int h0_in = c0 ? sp_row0<MODE>(c0, go, ge, iod1, acc_in) : 0;
            int lt[kEnCpl + 3];                                 // the letters of columns j - 1 .. j + 9 of the lane's first column j
#pragma unroll
            for (int t = 0; t < kEnCpl + 3; ++t) lt[t] = letter(c0 + lane * kEnCpl - 1 + t);
#pragma unroll
            for (int k = 0; k < kEnCpl; ++k) {
                const int p = lane * kEnCpl + k, j = c0 + 1 + p;
                rcode[k] = j <= n ? lt[k + 1] : 0;
                off[k] = (int)((uint32_t)(p + 1) * (uint32_t)ge - (uint32_t)go);
                iod[k] = io + sp_site(site, soff, 0, lt[k + 2], lt[k + 3]);      // io + don(j + 1): what opening an intron behind column j costs
                acc[k] = sp_site(site, soff, 16, lt[k], lt[k + 1]);             // acc(j)
                Hp[k] = sp_row0<MODE>(j, go, ge, iod1, acc[k]);
                Fp[k] = Hp[k] - go;
            }
            hleft = dpp_shr1(h0_in, Hp[kEnCpl - 1]);
        }
        const int32_t* in0 = hand + (size_t)(KEPT ? (c > 0 ? c - 1 : 0) : (c + 1) & 1) * NH * mpad;   // written by chunk c - 1; the third of each only where NH == 3
        const int32_t* in1 = in0 + mpad;
        const int32_t* in2 = in1 + mpad;
        int32_t* out0 = hand + (size_t)(KEPT ? c : c & 1) * NH * mpad;       // dereferenced by a chunk that hands on alone
        int32_t* out1 = out0 + mpad;
        int32_t* out2 = out1 + mpad;
        word_t* wsp = nullptr;
        if (FORM == EN_STORE && ws_ok) wsp = (word_t*)(prm.ws + pr.ws_off) + (size_t)c * m * 64;
        if (FORM == EN_TILE) wsp = tile;
        const int own = cols - lane * kEnCpl;                  // extend: register k holds a column of the reference while k < own
        int cv = (int)0x80000000, ci = 0, ck = 0;              // extend: this chunk's best of the lane

        for (int i0 = 0; i0 < mr; i0 += 64) {
            const bool mine = i0 + lane < mr;
            const int qv = mine ? ((int)qry[i0 + lane] & 31) : 0;
            int vin0 = 0, vin1 = 0, vin2 = 0, vout0 = 0, vout1 = 0, vout2 = 0;     // the NH values of rows i0 .. i0 + 63, row i0 + lane in this lane: in and out
            if (c > 0 && mine) {
                vin0 = in0[i0 + lane]; vin1 = in1[i0 + lane];
                if constexpr (NH == 3) vin2 = in2[i0 + lane];
            }
            const int rows = mr - i0 < 64 ? mr - i0 : 64;
            for (int rr = 0; rr < rows; ++rr) {
                const int i = i0 + rr + 1;
                const int qc = __builtin_amdgcn_readlane(qv, rr);
                const int* srow = smat + qc * 32;
                int T[kEnCpl], F[kEnCpl], D[kEnCpl], H[kEnCpl], E[kEnCpl];
                int F2[kEnCpl], E2[kEnCpl];                     // two pieces
                int N[kEnCpl], X[kEnCpl];                       // spliced
                // per model: the column in front of the chunk, this row -- its H (hin; spliced: and T, tin) and E (two pieces: E_1, E_2;
                // spliced: E, N) of the chunk's first column -- and then the row step
                int tin, hin;
                if constexpr (model == EN_ONE_PIECE) {
                    int ein;
                    if (c == 0) { hin = en_col0<MODE>(i, go, ge); ein = hin - go; }
                    else { hin = __builtin_amdgcn_readlane(vin0, rr); ein = __builtin_amdgcn_readlane(vin1, rr); }
                    const int E0 = pr_max(ein - ge, hin - go);
                    int v = 0;
#pragma unroll
                    for (int k = 0; k < kEnCpl; ++k) {
                        F[k] = pr_max(Hp[k] - go, Fp[k] - ge);
                        D[k] = (k ? Hp[k - 1] : hleft) + srow[rcode[k]];
                        T[k] = pr_max(D[k], F[k]);
                        const int xk = T[k] + off[k];
                        v = k ? pr_max(v, xk) : xk;
                    }
                    v = lane == 0 ? pr_max(v, E0) : v;
                    int u = dpp_shr1(E0, wave_prefix_max(v));                // lane 0 keeps E0
#pragma unroll
                    for (int k = 0; k < kEnCpl; ++k) {
                        E[k] = u - poff[k];
                        H[k] = pr_max(T[k], E[k]);
                        u = pr_max(u, T[k] + off[k]);
                    }
                } else if constexpr (model == EN_TWO_PIECE) {
                    int E0, E02;
                    if (c == 0) { hin = en2_col0<MODE>(i, prm); E0 = hin - go; E02 = hin - go2; }
                    else {
                        hin = __builtin_amdgcn_readlane(vin0, rr);
                        E0 = pr_max(__builtin_amdgcn_readlane(vin1, rr) - ge, hin - go);
                        E02 = pr_max(__builtin_amdgcn_readlane(vin2, rr) - ge2, hin - go2);
                    }
                    int v1 = 0, v2 = 0;
#pragma unroll
                    for (int k = 0; k < kEnCpl; ++k) {
                        F[k] = pr_max(Hp[k] - go, Fp[k] - ge);
                        F2[k] = pr_max(Hp[k] - go2, F2p[k] - ge2);
                        D[k] = (k ? Hp[k - 1] : hleft) + srow[rcode[k]];
                        T[k] = pr_max(pr_max(D[k], F[k]), F2[k]);
                        const int x1 = T[k] + off[k], x2 = T[k] + off2[k];
                        v1 = k ? pr_max(v1, x1) : x1;
                        v2 = k ? pr_max(v2, x2) : x2;
                    }
                    v1 = lane == 0 ? pr_max(v1, E0) : v1;
                    v2 = lane == 0 ? pr_max(v2, E02) : v2;
                    const int s1 = wave_prefix_max(v1), s2 = wave_prefix_max(v2);
                    int e1 = dpp_shr1(E0, s1) - base, e2 = dpp_shr1(E02, s2) - base2;        // lane 0 keeps E0_p (its base is 0)
#pragma unroll
                    for (int k = 0; k < kEnCpl; ++k) {
                        E[k] = e1; E2[k] = e2;
                        H[k] = pr_max(T[k], pr_max(e1, e2));
                        e1 = pr_max(e1 - ge, T[k] - go);
                        e2 = pr_max(e2 - ge2, T[k] - go2);
                    }
                } else {
                    int E0, N0;
                    if (c == 0) { tin = en_col0<MODE>(i, go, ge); hin = tin; E0 = tin - go; N0 = tin - iod_in; }
                    else {
                        tin = __builtin_amdgcn_readlane(vin0, rr);
                        const int e_in = __builtin_amdgcn_readlane(vin1, rr), nin = __builtin_amdgcn_readlane(vin2, rr);
                        hin = pr_max(tin, pr_max(e_in, nin - acc_in));
                        E0 = pr_max(e_in - ge, tin - go);
                        N0 = pr_max(nin, tin - iod_in);
                    }
                    int ve = 0, vn = 0;
#pragma unroll
                    for (int k = 0; k < kEnCpl; ++k) {
                        F[k] = pr_max(Hp[k] - go, Fp[k] - ge);
                        D[k] = (k ? Hp[k - 1] : hleft) + srow[rcode[k]];
                        T[k] = pr_max(D[k], F[k]);
                        X[k] = T[k] - iod[k];
                        const int xe = T[k] + off[k];
                        ve = k ? pr_max(ve, xe) : xe;
                        vn = k ? pr_max(vn, X[k]) : X[k];
                    }
                    ve = lane == 0 ? pr_max(ve, E0) : ve;
                    vn = lane == 0 ? pr_max(vn, N0) : vn;
                    const int se = wave_prefix_max(ve), sn = wave_prefix_max(vn);
                    int e = dpp_shr1(E0, se) - base, u = dpp_shr1(N0, sn);   // lane 0 keeps E0 (its base is 0) and N0
#pragma unroll
                    for (int k = 0; k < kEnCpl; ++k) {
                        E[k] = e; N[k] = u;
                        H[k] = pr_max(T[k], pr_max(e, u - acc[k]));
                        e = pr_max(e - ge, T[k] - go);
                        u = pr_max(u, X[k]);
                    }
                }
                const int nleft = dpp_shr1(hin, H[kEnCpl - 1]);          // H[i][first own column - 1]
                if (STORE) {
                    if constexpr (model == EN_ONE_PIECE) {
                        uint32_t w = 0;
#pragma unroll
                        for (int k = 0; k < kEnCpl; ++k) {
                            const int left = k ? H[k - 1] : nleft;
                            const uint32_t src = H[k] == D[k] ? 0u : (H[k] == E[k] ? 1u : 2u);
                            const uint32_t nib = src | (E[k] == left - go ? 4u : 0u) | (F[k] == Hp[k] - go ? 8u : 0u);
                            w |= nib << (4 * k);
                        }
                        if (wsp && lane < L) wsp[(size_t)(i - 1) * L + lane] = w;
                    } else if constexpr (model == EN_TWO_PIECE) {
                        uint32_t w[2] = {0u, 0u};
#pragma unroll
                        for (int k = 0; k < kEnCpl; ++k) {
                            const int left = k ? H[k - 1] : nleft;
                            const uint32_t src = H[k] == D[k] ? 0u : (H[k] == E[k] ? 1u : (H[k] == E2[k] ? 2u : (H[k] == F[k] ? 3u : 4u)));
                            const uint32_t b = src | (E[k] == left - go ? 8u : 0u) | (E2[k] == left - go2 ? 16u : 0u) |
                                               (F[k] == Hp[k] - go ? 32u : 0u) | (F2[k] == Hp[k] - go2 ? 64u : 0u);
                            w[k >> 2] |= b << (8 * (k & 3));
                        }
                        if (wsp && lane < L) wsp[(size_t)(i - 1) * L + lane] = make_uint2(w[0], w[1]);
                    } else {
                        const int tleft = dpp_shr1(tin, T[kEnCpl - 1]);      // T[i][first own column - 1]
                        const int xleft = dpp_shr1(tin - iod_in, X[kEnCpl - 1]);
                        uint32_t w[2] = {0u, 0u};
#pragma unroll
                        for (int k = 0; k < kEnCpl; ++k) {
                            const int tl = k ? T[k - 1] : tleft, xl = k ? X[k - 1] : xleft;
                            const uint32_t src = H[k] == D[k] ? 0u : (H[k] == E[k] ? 1u : (H[k] == N[k] - acc[k] ? 2u : 3u));
                            const uint32_t b = src | (T[k] == D[k] ? 0u : 4u) | (E[k] == tl - go ? 8u : 0u) | (N[k] == xl ? 16u : 0u) |
                                               (F[k] == Hp[k] - go ? 32u : 0u);
                            w[k >> 2] |= b << (8 * (k & 3));
                        }
                        if (wsp && lane < L) wsp[(size_t)(i - 1) * L + lane] = make_uint2(w[0], w[1]);
                    }
                }
                if (FORM != EN_TILE && !last) {
                    // what lane 63 hands on of its last column: H (spliced: T), E, and E_2 or N
                    const int s0 = __builtin_amdgcn_readlane(model == EN_SPLICED ? T[kEnCpl - 1] : H[kEnCpl - 1], 63);
                    const int s1 = __builtin_amdgcn_readlane(E[kEnCpl - 1], 63);
                    int s2 = 0;
                    if constexpr (model == EN_TWO_PIECE) s2 = __builtin_amdgcn_readlane(E2[kEnCpl - 1], 63);
                    if constexpr (model == EN_SPLICED) s2 = __builtin_amdgcn_readlane(N[kEnCpl - 1], 63);
                    vout0 = lane == rr ? s0 : vout0;                     // lane rr keeps row i0 + rr: one coalesced store per 64 rows
                    vout1 = lane == rr ? s1 : vout1;
                    if constexpr (NH == 3) vout2 = lane == rr ? s2 : vout2;
                }
                if (FORM != EN_TILE && MODE == EN_EXTEND) {
#pragma unroll
                    for (int k = 0; k < kEnCpl; ++k)
                        if (k < own && H[k] > cv) { cv = H[k]; ci = i; ck = k; }
                }
                if (FORM != EN_TILE && (MODE == EN_SEMIGLOBAL || MODE == EN_OVERLAP || MODE == EN_PREFIX) && i == m) {
                    int bv = (int)0x80000000, bj = 0x7fffffff;
#pragma unroll
                    for (int k = 0; k < kEnCpl; ++k) {
                        const int j = c0 + 1 + lane * kEnCpl + k;
                        if (j <= n && H[k] > bv) { bv = H[k]; bj = j; }
                    }
#pragma unroll
                    for (int d = 1; d < 64; d <<= 1) {
                        const int v2 = __shfl_xor(bv, d), j2 = __shfl_xor(bj, d);
                        const bool take = v2 > bv || (v2 == bv && j2 < bj);
                        bv = take ? v2 : bv; bj = take ? j2 : bj;
                    }
                    if (bv > row_best) { row_best = bv; row_j = bj; }
                }
                if (FORM != EN_TILE && last && (MODE == EN_OVERLAP || i == m)) {
                    int hn = H[0];
#pragma unroll
                    for (int k = 1; k < kEnCpl; ++k) hn = k == kn ? H[k] : hn;
                    if (i == m) corner = hn;
                    else if (hn > col_best) { col_best = hn; col_i = i; }    // meaningful in lane ln
                }
#pragma unroll
                for (int k = 0; k < kEnCpl; ++k) {
                    Hp[k] = H[k]; Fp[k] = F[k];
                    if constexpr (model == EN_TWO_PIECE) F2p[k] = F2[k];
                }
                hleft = nleft;
            }
            if (FORM != EN_TILE && !last && mine) {
                out0[i0 + lane] = vout0; out1[i0 + lane] = vout1;
                if constexpr (NH == 3) out2[i0 + lane] = vout2;
            }
        }
        if (FORM != EN_TILE && MODE == EN_EXTEND) {
            const bool take = cv > ext_v || (cv == ext_v && ci < ext_i);
            ext_v = take ? cv : ext_v; ext_i = take ? ci : ext_i; ext_j = take ? c0 + 1 + lane * kEnCpl + ck : ext_j;
        }
        if (FORM != EN_TILE && !last) {      // the next chunk reads what other lanes of this wave stored
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            __syncthreads();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        }
    }
    if (FORM == EN_TILE) return;                     // the tile form tracks no end cell and writes no row
    corner = __shfl(corner, ln); col_best = __shfl(col_best, ln); col_i = __shfl(col_i, ln);
    int score, ei, ej;
    if (MODE == EN_GLOBAL) { score = corner; ei = m; ej = n; }
    else if (MODE == EN_EXTEND) {
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int v2 = __shfl_xor(ext_v, d), i2 = __shfl_xor(ext_i, d), j2 = __shfl_xor(ext_j, d);
            const bool take = v2 > ext_v || (v2 == ext_v && (i2 < ext_i || (i2 == ext_i && j2 < ext_j)));
            ext_v = take ? v2 : ext_v; ext_i = take ? i2 : ext_i; ext_j = take ? j2 : ext_j;
        }
        score = ext_v; ei = ext_i; ej = ext_j;
    }
    else if (MODE == EN_SEMIGLOBAL || MODE == EN_PREFIX || row_best >= col_best) { score = row_best; ei = m; ej = row_j; }     // last-row cells before last-column cells
    else { score = col_best; ei = col_i; ej = n; }
    if (lane == 0) {
        int32_t* row = prm.rows + (size_t)(first + x) * 8;
        row[0] = score;
        row[1] = en_anchored(MODE) ? 0 : -1;                      // begins: the walk's, unless the mode fixes them
        row[2] = ej - 1;
        row[3] = MODE == EN_OVERLAP ? -1 : 0;
        row[4] = ei - 1;
        row[5] = 0;
        row[6] = 0;
        row[7] = (FORM == EN_STORE && !ws_ok) ? EN_ST_NO_WALK : 0;
        if constexpr (FORM == EN_KEEP) {              // the fresh record: the walk starts at the end cell, in its chunk
            rec[EN_REC_DONE] = 0; rec[EN_REC_CHUNK] = ej > 0 ? (ej - 1) / kEnChunk : 0; rec[EN_REC_I] = ei; rec[EN_REC_J] = ej;
            rec[EN_REC_STATE] = 0; rec[EN_REC_CUR] = -1; rec[EN_REC_RUN] = 0; rec[EN_REC_NOPS] = 0; rec[EN_REC_STEPS] = ei + ej + 2;
        }
    }
}

// one lane per pair: pr_walk over what the storing form left, where EnCells says it lies.  Spliced reads a lane's 8 bytes of a row at
// a time: an intron is thousands of steps along one row, and each of its words is loaded once.
template <typename Prm>
__global__ void ssw_ends_walk_kernel(const Prm prm, int first, int count)
{
    constexpr int model = EnModel<Prm>::model;
    typedef typename EnModel<Prm>::cell_t cell_t;
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= count || first + x >= prm.npairs) return;
    const EnPair pr = prm.pairs[first + x];
    const int m = pr.m, n = pr.n;
    if (m <= 0 || n <= 0) return;
    int32_t* row = prm.rows + (size_t)(first + x) * 8;
    if (row[7] != 0) return;                                     // unwritten, or without stored decisions: fetch reports it
    EnCells<cell_t> cells(m, n);
    if (pr.ws_off < 0 || (sizeof(cell_t) == 8 && (pr.ws_off & 7) != 0) || pr.ws_off + cells.bytes() > prm.ws_cap ||
        pr.cig_off < 0 || pr.cig_off + pr.cig_cap > prm.cigar_cap) { row[7] = EN_ST_NO_WALK; return; }
    cells.ws = (const cell_t*)(prm.ws + pr.ws_off);
    if constexpr (model == EN_SPLICED) {
        const int8_t* ref = prm.ref + pr.r_off;
        const int soff = (prm.strand && prm.strand[first + x] < 0) ? 32 : 0;
        auto letter = [&](int pos) -> int { return (pos >= 0 && pos < n) ? ((int)ref[pos] & 31) : 4; };
        pr_walk<model>(row, prm.mode, m, n, prm.cigar + pr.cig_off, pr.cig_cap, cells, [&](int j) -> int {
            // the run of j letters on row 0: D (2) if the deletion is not dearer, else N (3)
            const int64_t del = (int64_t)prm.go + (int64_t)(j - 1) * prm.ge;
            const int64_t intron = (int64_t)prm.io + sp_site(prm.site, soff, 0, letter(0), letter(1)) + sp_site(prm.site, soff, 16, letter(j - 2), letter(j - 1));
            return del <= intron ? 2 : 3;
        });
    }
    else pr_walk<model>(row, prm.mode, m, n, prm.cigar + pr.cig_off, pr.cig_cap, cells);
}

// The recompute route's walk, one lane per pair: a round of pr_walk_round over the tile the tile form has just filled for the
// chunk in the pair's record.  Chunk and row limit are clamped as the tile form clamps them; a record that disagrees is refused there.
template <typename Prm>
__global__ void ssw_ends_rewalk_kernel(const Prm prm, int first, int count, int last_round)
{
    constexpr int model = EnModel<Prm>::model, NH = EnModel<Prm>::NH;
    typedef typename EnModel<Prm>::cell_t cell_t;
    typedef typename EnModel<Prm>::word_t word_t;
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= count || first + x >= prm.npairs) return;
    const EnPair pr = prm.pairs[first + x];
    const int m = pr.m, n = pr.n;
    if (m <= 0 || n <= 0) return;
    int32_t* row = prm.rows + (size_t)(first + x) * 8;
    if (row[7] != 0) return;                                     // unwritten, or refused in an earlier round: fetch reports it
    const EnKept lay(m, n, NH, (int)sizeof(word_t));
    if (!lay.fits(pr.ws_off, prm.ws_cap) || pr.cig_off < 0 || pr.cig_off + pr.cig_cap > prm.cigar_cap) { row[7] = EN_ST_NO_WALK; return; }
    int32_t* rec = (int32_t*)(prm.ws + pr.ws_off + lay.rec_off);
    if (rec[EN_REC_DONE] != 0) return;
    const int nchunks = (n + kEnChunk - 1) / kEnChunk;
    int c = rec[EN_REC_CHUNK], ilim = rec[EN_REC_I];
    c = c < 0 ? 0 : (c > nchunks - 1 ? nchunks - 1 : c);
    ilim = ilim > m ? m : (ilim < 0 ? 0 : ilim);
    EnTile<cell_t> cells(m, n, c, ilim);
    cells.ws = (const cell_t*)(prm.ws + pr.ws_off + lay.plane_off);
    if constexpr (model == EN_SPLICED) {
        const int8_t* ref = prm.ref + pr.r_off;
        const int soff = (prm.strand && prm.strand[first + x] < 0) ? 32 : 0;
        auto letter = [&](int pos) -> int { return (pos >= 0 && pos < n) ? ((int)ref[pos] & 31) : 4; };
        pr_walk_round<model>(rec, row, prm.mode, m, n, prm.cigar + pr.cig_off, pr.cig_cap, cells, c, last_round != 0, [&](int j) -> int {
            const int64_t del = (int64_t)prm.go + (int64_t)(j - 1) * prm.ge;
            const int64_t intron = (int64_t)prm.io + sp_site(prm.site, soff, 0, letter(0), letter(1)) + sp_site(prm.site, soff, 16, letter(j - 2), letter(j - 1));
            return del <= intron ? 2 : 3;
        });
    }
    else pr_walk_round<model>(rec, row, prm.mode, m, n, prm.cigar + pr.cig_off, pr.cig_cap, cells, c, last_round != 0);
}

#ifdef CLH_EN_RETRACE
// the recompute route's launchers, an object of their own (the Makefile builds this file twice): 30 more instantiations of the body
template <typename Prm, int FORM>
static hipError_t en_launch_form(const Prm& p, int first, int count, hipStream_t st)
{
    if (p.mode == EN_GLOBAL) hipLaunchKernelGGL((ssw_ends_kernel<Prm, EN_GLOBAL, FORM>), dim3(count), dim3(64), 0, st, p, first, count);
    else if (p.mode == EN_SEMIGLOBAL) hipLaunchKernelGGL((ssw_ends_kernel<Prm, EN_SEMIGLOBAL, FORM>), dim3(count), dim3(64), 0, st, p, first, count);
    else if (p.mode == EN_OVERLAP) hipLaunchKernelGGL((ssw_ends_kernel<Prm, EN_OVERLAP, FORM>), dim3(count), dim3(64), 0, st, p, first, count);
    else if (p.mode == EN_PREFIX) hipLaunchKernelGGL((ssw_ends_kernel<Prm, EN_PREFIX, FORM>), dim3(count), dim3(64), 0, st, p, first, count);
    else if (p.mode == EN_EXTEND) hipLaunchKernelGGL((ssw_ends_kernel<Prm, EN_EXTEND, FORM>), dim3(count), dim3(64), 0, st, p, first, count);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

// the keeping score pass of a share, then `rounds` times the tile form and a round of the walk, in stream order
template <typename Prm>
static hipError_t en_launch_retrace(const Prm& p, int first, int count, int rounds, hipStream_t stream)
{
    if (count <= 0) return hipSuccess;
    hipError_t e = en_launch_form<Prm, EN_KEEP>(p, first, count, stream);
    for (int r = 0; r < rounds && e == hipSuccess; ++r) {
        e = en_launch_form<Prm, EN_TILE>(p, first, count, stream);
        if (e != hipSuccess) break;
        hipLaunchKernelGGL(ssw_ends_rewalk_kernel<Prm>, dim3((count + 63) / 64), dim3(64), 0, stream, p, first, count, r == rounds - 1 ? 1 : 0);
        e = hipGetLastError();
    }
    return e;
}

hipError_t launch_ssw_ends_retrace(const EnParams& p, int first, int count, int rounds, hipStream_t stream) { return en_launch_retrace(p, first, count, rounds, stream); }
hipError_t launch_ssw_ends2_retrace(const En2Params& p, int first, int count, int rounds, hipStream_t stream) { return en_launch_retrace(p, first, count, rounds, stream); }
hipError_t launch_ssw_spliced_retrace(const SpParams& p, int first, int count, int rounds, hipStream_t stream) { return en_launch_retrace(p, first, count, rounds, stream); }
#else
template <typename Prm, int MODE>
static void en_launch_mode(const Prm& p, bool store, int first, int count, hipStream_t st)
{
    if (store) hipLaunchKernelGGL((ssw_ends_kernel<Prm, MODE, EN_STORE>), dim3(count), dim3(64), 0, st, p, first, count);
    else hipLaunchKernelGGL((ssw_ends_kernel<Prm, MODE, EN_SCORE>), dim3(count), dim3(64), 0, st, p, first, count);
}

template <typename Prm>
static hipError_t en_launch(const Prm& p, bool store, int first, int count, hipStream_t stream)
{
    if (count <= 0) return hipSuccess;
    if (p.mode == EN_GLOBAL) en_launch_mode<Prm, EN_GLOBAL>(p, store, first, count, stream);
    else if (p.mode == EN_SEMIGLOBAL) en_launch_mode<Prm, EN_SEMIGLOBAL>(p, store, first, count, stream);
    else if (p.mode == EN_OVERLAP) en_launch_mode<Prm, EN_OVERLAP>(p, store, first, count, stream);
    else if (p.mode == EN_PREFIX) en_launch_mode<Prm, EN_PREFIX>(p, store, first, count, stream);
    else if (p.mode == EN_EXTEND) en_launch_mode<Prm, EN_EXTEND>(p, store, first, count, stream);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

template <typename Prm>
static hipError_t en_launch_walk(const Prm& p, int first, int count, hipStream_t stream)
{
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(ssw_ends_walk_kernel<Prm>, dim3((count + 63) / 64), dim3(64), 0, stream, p, first, count);
    return hipGetLastError();
}

hipError_t launch_ssw_ends(const EnParams& p, bool store, int first, int count, hipStream_t stream) { return en_launch(p, store, first, count, stream); }
hipError_t launch_ssw_ends2(const En2Params& p, bool store, int first, int count, hipStream_t stream) { return en_launch(p, store, first, count, stream); }
hipError_t launch_ssw_spliced(const SpParams& p, bool store, int first, int count, hipStream_t stream) { return en_launch(p, store, first, count, stream); }
hipError_t launch_ssw_ends_walk(const EnParams& p, int first, int count, hipStream_t stream) { return en_launch_walk(p, first, count, stream); }
hipError_t launch_ssw_ends2_walk(const En2Params& p, int first, int count, hipStream_t stream) { return en_launch_walk(p, first, count, stream); }
hipError_t launch_ssw_spliced_walk(const SpParams& p, int first, int count, hipStream_t stream) { return en_launch_walk(p, first, count, stream); }
#endif

}  // namespace clh
