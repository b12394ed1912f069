// ssw_pairs.h -- what K1g (ssw_ends.hip) and K1gb (ssw_band.hip) share on the device: the LDS matrix of their score kernels and the
// walk back over the stored decisions.  The walk (pr_walk_steps, entered as pr_walk<MODEL> over everything that was stored and as
// pr_walk_round<MODEL> over one chunk's plane at a time) is one body for the three gap models (one piece, two pieces, intron gaps): the
// frame is written once, and what a model has of its own is a few constants (PrModel) and, for spliced, two branches under
// `if constexpr`.  Where the decisions of a cell lie is the geometry's: EnCells and EnTile (K1g) and BdCells (K1gb), which the walk
// takes as a functor.  They check rows, columns and the plane's bounds themselves and state the plane's size, and the walk kernels' guards use
// that same expression.  Walk and locators are __host__ __device__: tests/walk_host.hip runs them on the CPU over random planes.
// (Each of the two score kernels is one template body for all its gap models.  The storing side of the layout, the decision bits of
// a cell and the end cell's argmax over the wave stay written out there: as helpers they changed the register allocation of the
// storing forms -- LABNOTES.md 16 and 20 have the tables.  The walk is one lane per pair, far from the row loop.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "clh_device.h"

namespace clh {

__device__ __forceinline__ int pr_max(int a, int b) { return a > b ? a : b; }

// smat[query code][reference code], 32 x 32 ints in LDS, zero outside the n_mat x n_mat matrix; the whole workgroup (one wave) calls it
__device__ __forceinline__ void pr_load_matrix(int* smat, const int8_t* mat, int n_mat, int lane)
{
    for (int k = lane; k < 32 * 32; k += 64) {
        const int qc = k >> 5, rc = k & 31;
        smat[k] = (qc < n_mat && rc < n_mat) ? (int)mat[rc * n_mat + qc] : 0;
    }
    __syncthreads();
}

// The gap model of a parameter block (EnModel in ssw_ends.hip, BdModel in ssw_band.hip name it), and what it means to the walk.
// A stored cell holds H's source in its low bits -- 0 the diagonal, then the model's gap states in the order of its tie rule -- and
// above them one "opened here" bit per gap state, in the same order:
//     one piece   4 bits   source 0..1: 1 E, 2 F;                     bit 2 E, bit 3 F
//     two pieces  a byte   source 0..2: 1 E_1, 2 E_2, 3 F_1, 4 F_2;   bits 3..6 E_1, E_2, F_1, F_2
//     spliced     a byte   source 0..1: 1 E, 2 N, 3 F;                bit 2 T's source (0 diagonal, 1 F);  bits 3..5 E, N, F
// The first n_ref gap states take a reference letter (op D, 2; spliced N: op N, 3), the others up to n_gap a query letter (op I, 1).
enum { EN_ONE_PIECE, EN_TWO_PIECE, EN_SPLICED };
template <int MODEL> struct PrModel {
    static constexpr uint32_t src_mask = MODEL == EN_TWO_PIECE ? 7u : 3u;
    static constexpr int n_ref = MODEL == EN_ONE_PIECE ? 1 : 2, n_gap = MODEL == EN_ONE_PIECE ? 2 : (MODEL == EN_TWO_PIECE ? 4 : 3);
    static constexpr uint32_t open1 = MODEL == EN_ONE_PIECE ? 4u : 8u;      // "opened here" of gap state s is open1 << (s - 1)
    static constexpr int T = 4;                                             // spliced alone: the state H without a reference gap
};

struct PrRow0D { __host__ __device__ int operator()(int) const { return 2; } };     // the run on row 0 is a deletion

// One lane walks one pair's stored decisions back from the end cell its score kernel left in `row`, writes the CIGAR (BAM ops M 0,
// I 1, D 2, N 3; equal neighbours merged) and the begins; at most i + j + 2 steps, each of which consumes a letter.  The tie rule is
// the order of the sources; a gap state takes its first letter from the cell that names it and is left as soon as its own "opened
// here" is set.  cell(i, j) gives the stored bits of cell (i, j), or -1 where the cell is outside what was stored.  A gap state that
// stands on row 0 or column 0, a source that names no state, a CIGAR of more than cig_cap runs, a walk that does not stop: whatever
// does not add up sets EN_ST_NO_WALK, which fetch reports.  The caller has checked that `out` holds cig_cap ops.
// Spliced: on leaving E or N the walk is in state T: the diagonal if T equals it, else F, never E or N again, so that no D stands
// next to an N.  cell.run_left(i, j, bit, &opened) gives how many cells of the E or N run that stands on (i, j) lie in the stored word
// of that cell, from column j leftwards up to and including the first whose `bit` ("opened here") is set, or 0 outside what was stored:
// an intron is thousands of cells along one row, taken 8 at a step.  row0_op(j) names the op of the one run of j letters that the
// anchored stop on row 0 emits; the other models neither have run_left nor pass a row0_op.
// The walk is written once, as a round over a record (pr_walk_steps): rec holds where the walk stands -- (i, j), the state, the open
// run (cur, run), the ops written and the steps left -- and TILED says whether `cell` is one chunk's plane (K1g's recompute route,
// pr_walk_round) or everything that was stored (pr_walk, whose record is a local that never leaves the registers).  A tiled round
// that needs a cell left of its tile (0 < j <= c0) saves the record, names chunk c - 1 and returns: the open run is in the record,
// so a run across a chunk edge is one op, and so are the steps left, so the budget is spent once.  A record that does not add up for
// the tile it is resumed on, and a pair still open when `last_round` ends, is EN_ST_NO_WALK.
enum { EN_REC_DONE, EN_REC_CHUNK, EN_REC_I, EN_REC_J, EN_REC_STATE, EN_REC_CUR, EN_REC_RUN, EN_REC_NOPS, EN_REC_STEPS, kEnRecWords = 12 };
template <int MODEL, bool TILED, typename Cell, typename Row0>
__host__ __device__ __forceinline__ void pr_walk_steps(int32_t* rec, int32_t* row, int mode, int m, int n, uint32_t* out, int cig_cap, Cell& cell,
                                                       int c, bool last_round, Row0 row0_op)
{
    typedef PrModel<MODEL> M;
    const int c0 = TILED ? c * kEnChunk : 0;
    int i = rec[EN_REC_I], j = rec[EN_REC_J], state = rec[EN_REC_STATE], cur = rec[EN_REC_CUR], run = rec[EN_REC_RUN], nops = rec[EN_REC_NOPS];
    int steps = rec[EN_REC_STEPS];
    if constexpr (TILED) {
        rec[EN_REC_DONE] = 1;                                    // unless this round suspends
        if (rec[EN_REC_CHUNK] != c || c < 0 || i < 0 || i > m || j < (c ? c0 + 1 : 0) || j > n || j > c0 + kEnChunk ||
            state < 0 || (state > M::n_gap && !(MODEL == EN_SPLICED && state == M::T)) || cur < -1 || cur > 3 || run < 0 || (run > 0 && cur < 0) ||
            nops < 0 || nops > cig_cap || steps < 0 || steps > m + n + 2) { row[7] = EN_ST_NO_WALK; return; }
    }
    bool bad = false, done = false;
    auto emit = [&](int op, int k) {
        if (k <= 0) return;
        if (op == cur) { run += k; return; }
        if (run) { if (nops < cig_cap) out[nops++] = ((uint32_t)run << 4) | (uint32_t)cur; else bad = true; }
        cur = op; run = k;
    };
    for (; steps > 0 && !done; --steps) {
        if ((state == 0 || (MODEL == EN_SPLICED && state == M::T)) && (i == 0 || j == 0)) {     // on column 0 T is H; state T never stands on row 0
            if (en_anchored(mode)) { if (j > 0) emit(row0_op(j), j); emit(1, i); i = 0; j = 0; }      // prefix and extend stop at (0, 0) as global does
            else if (mode == EN_SEMIGLOBAL && j == 0) { emit(1, i); i = 0; }
            done = true;
            break;
        }
        if constexpr (TILED) {
            if (j > 0 && j <= c0) {                              // the cell lies in the chunk before this one: the next round's
                if (last_round) break;
                rec[EN_REC_CHUNK] = c - 1; rec[EN_REC_I] = i; rec[EN_REC_J] = j; rec[EN_REC_STATE] = state; rec[EN_REC_CUR] = cur;
                rec[EN_REC_RUN] = run; rec[EN_REC_NOPS] = nops; rec[EN_REC_STEPS] = steps;
                if (bad) row[7] = EN_ST_NO_WALK; else rec[EN_REC_DONE] = 0;
                return;
            }
        }
        const int at = cell(i, j);                               // -1 on row 0 and column 0: a gap state on the boundary does not add up
        if (at < 0) { bad = true; break; }
        const uint32_t b = (uint32_t)at;
        if (state == 0) {
            state = (int)(b & M::src_mask);                      // a gap state takes its first letter from this same cell
            if (state == 0) { emit(0, 1); --i; --j; continue; }
        } else if (MODEL == EN_SPLICED && state == M::T) {
            if (!(b & 4u)) { emit(0, 1); --i; --j; state = 0; continue; }
            state = 3;
        }
        const uint32_t open = (M::open1 >> 1) << state;          // state >= 1 here
        if (state <= M::n_ref) {
            if constexpr (MODEL == EN_SPLICED) {
                bool opened = false;
                const int k = cell.run_left(i, j, open, &opened);
                if (k <= 0 || k > j) { bad = true; break; }
                emit(state == 1 ? 2 : 3, k); j -= k;
                if (opened) state = M::T;
            }
            else { emit(2, 1); --j; if (b & open) state = 0; }
        }
        else if (state <= M::n_gap) { emit(1, 1); --i; if (b & open) state = 0; }
        else { bad = true; break; }
    }
    emit(-2, 1);                                                 // flush the last run
    if (bad || !done) { row[7] = EN_ST_NO_WALK; return; }
    for (int a = 0, z = nops - 1; a < z; ++a, --z) { const uint32_t w = out[a]; out[a] = out[z]; out[z] = w; }
    row[1] = j; row[3] = i; row[5] = nops;
}

// the walk over everything that was stored, from the end cell in `row`
template <int MODEL, typename Cell, typename Row0 = PrRow0D>
__host__ __device__ __forceinline__ void pr_walk(int32_t* row, int mode, int m, int n, uint32_t* out, int cig_cap, Cell& cell, Row0 row0_op = Row0())
{
    const int i = row[4] + 1, j = row[2] + 1;
    if (i < 0 || i > m || j < 0 || j > n) { row[7] = EN_ST_NO_WALK; return; }
    int32_t rec[kEnRecWords] = {0, 0, i, j, 0, -1, 0, 0, i + j + 2};
    pr_walk_steps<MODEL, false>(rec, row, mode, m, n, out, cig_cap, cell, 0, true, row0_op);
}

// one round of the walk over the tile of chunk c (EnTile); rec is the pair's resume record, which the keeping score pass leaves fresh:
// the end cell, its chunk, state 0, no open run, i + j + 2 steps
template <int MODEL, typename Cell, typename Row0 = PrRow0D>
__host__ __device__ __forceinline__ void pr_walk_round(int32_t* rec, int32_t* row, int mode, int m, int n, uint32_t* out, int cig_cap, Cell& cell,
                                                       int c, bool last_round, Row0 row0_op = Row0())
{
    if (rec[EN_REC_DONE] != 0) return;
    pr_walk_steps<MODEL, true>(rec, row, mode, m, n, out, cig_cap, cell, c, last_round, row0_op);
}

// Where the decisions of cell (i, j) lie in what K1g's storing form left of a pair: chunk after chunk, per chunk row after row, a
// word of kEnCpl cells per lane that owns a column, nwords of them.  Word is what the walk loads: uint32_t, a word of half-bytes; uint8_t,
// one byte of a word of bytes; uint2, a word of bytes, held: a run along a row loads each word once.  The constructor is given
// the pair, the caller checks that bytes() lie inside the workspace and sets ws.  -1 outside rows 1..m and columns 1..n, which is the
// plane exactly: the word of such a cell has an index below nwords (chunk by chunk: (i - 1) L + p / kEnCpl < m L).
template <typename Word>
struct EnCells {
    const Word* ws = nullptr;
    int m, n, nchunks, llast;
    int64_t nwords, held = -1;
    Word word;                                               // uint2 alone: the word loaded last, and its index
    __host__ __device__ EnCells(int m_, int n_) : m(m_), n(n_), nchunks((n_ + kEnChunk - 1) / kEnChunk), word()
    {
        llast = (n - (nchunks - 1) * kEnChunk + kEnCpl - 1) / kEnCpl;
        nwords = (int64_t)m * ((int64_t)64 * (nchunks - 1) + llast);
    }
    __host__ __device__ int64_t bytes() const { return (sizeof(Word) == 4 ? 4 : 8) * nwords; }
    // the index of the lane's word that holds cell (i, j), *k the cell's place in it; -1 outside the plane
    __host__ __device__ int64_t locate(int i, int j, int* k) const
    {
        const uint32_t r = (uint32_t)(i - 1), c = (uint32_t)(j - 1);                              // unsigned: row 0 and column 0 wrap, shifts and masks
        if (r >= (uint32_t)m || c >= (uint32_t)n) return -1;
        const uint32_t ch = c / kEnChunk, p = c % kEnChunk;
        const int L = (int)ch == nchunks - 1 ? llast : 64;
        *k = (int)(p % kEnCpl);
        return (int64_t)ch * m * 64 + (int64_t)r * L + p / kEnCpl;
    }
    __host__ __device__ void hold(int64_t wi)
    {
        static_assert(sizeof(Word) == 8, "only the uint2 functor holds a word");
        if (wi != held) { word = ws[wi]; held = wi; }
    }
    __host__ __device__ int operator()(int i, int j)
    {
        int k;
        const int64_t wi = locate(i, j, &k);
        if (wi < 0) return -1;
        if constexpr (sizeof(Word) == 4) return (int)((ws[wi] >> (4 * k)) & 15u);
        else if constexpr (sizeof(Word) == 1) return (int)ws[wi * kEnCpl + k];
        else { hold(wi); return (int)((((k & 4) ? word.y : word.x) >> (8 * (k & 3))) & 255u); }
    }
    __host__ __device__ int run_left(int i, int j, uint32_t bit, bool* opened)      // pr_walk states it
    {
        static_assert(sizeof(Word) == 8, "run_left reads the held uint2");
        int k;
        const int64_t wi = locate(i, j, &k);
        if (wi < 0) return 0;
        hold(wi);
        const uint64_t both = ((uint64_t)word.y << 32) | word.x;
        const uint64_t set = both & (0x0101010101010101ull * bit) & (~0ull >> (8 * (7 - k)));      // "opened here" of columns 0 .. k of the word
        *opened = set != 0;
        return set ? k - (63 - __builtin_clzll(set)) / 8 + 1 : k + 1;
    }
};

// The recompute route of K1g (ssw_ends.hip): what a pair holds in its share of the workspace in place of the whole plane.  First the
// last column of every chunk but the last, slot c written by chunk c of the keeping score pass (NH int32 values per row, rows rounded
// up to 64: `slot` bytes each); then the plane of one chunk, which the tile form fills for the rows the walk can still reach (a word
// per lane and row, as EnCells has a chunk: room for all m rows of 64 lanes); then the walk's resume record.  Host and kernels size
// and check the block with this one expression.
struct EnKept {
    int64_t slot, plane_off, rec_off, total;                 // bytes
    __host__ __device__ EnKept(int m, int n, int nh, int word_bytes)
    {
        const int64_t mpad = ((int64_t)m + 63) & ~(int64_t)63, nchunks = ((int64_t)n + kEnChunk - 1) / kEnChunk;
        slot = 4 * nh * mpad;
        plane_off = slot * (nchunks - 1);
        rec_off = plane_off + (int64_t)word_bytes * m * 64;
        total = (rec_off + 4 * kEnRecWords + 15) & ~(int64_t)15;
    }
    __host__ __device__ bool fits(int64_t ws_off, int64_t ws_cap) const { return ws_off >= 0 && (ws_off & 15) == 0 && ws_off + total <= ws_cap; }
};

// EnCells for the plane of one chunk: rows 1..ilim of chunk c of the pair, the words of a row side by side as the tile form stores
// them.  -1 above the row limit and left or right of the chunk: the word of any other cell has an index below ilim L <= 64 m.
template <typename Word>
struct EnTile {
    const Word* ws = nullptr;
    int c0, cols, L, ilim;
    int64_t held = -1;
    Word word;
    __host__ __device__ EnTile(int m, int n, int c, int ilim_) : c0(c * kEnChunk), ilim(ilim_ < m ? ilim_ : m), word()
    {
        cols = n - c0 < kEnChunk ? n - c0 : kEnChunk;
        L = (cols + kEnCpl - 1) / kEnCpl;
    }
    __host__ __device__ int64_t locate(int i, int j, int* k) const
    {
        const uint32_t r = (uint32_t)(i - 1), p = (uint32_t)(j - 1 - c0);                         // unsigned: what lies above or left wraps
        if (r >= (uint32_t)ilim || cols <= 0 || p >= (uint32_t)cols) return -1;
        *k = (int)(p % kEnCpl);
        return (int64_t)r * L + p / kEnCpl;
    }
    __host__ __device__ void hold(int64_t wi)
    {
        static_assert(sizeof(Word) == 8, "only the uint2 functor holds a word");
        if (wi != held) { word = ws[wi]; held = wi; }
    }
    __host__ __device__ int operator()(int i, int j)
    {
        int k;
        const int64_t wi = locate(i, j, &k);
        if (wi < 0) return -1;
        if constexpr (sizeof(Word) == 4) return (int)((ws[wi] >> (4 * k)) & 15u);
        else if constexpr (sizeof(Word) == 1) return (int)ws[wi * kEnCpl + k];
        else { hold(wi); return (int)((((k & 4) ? word.y : word.x) >> (8 * (k & 3))) & 255u); }
    }
    __host__ __device__ int run_left(int i, int j, uint32_t bit, bool* opened)      // ends at the word's first cell, hence at the tile's left edge
    {
        static_assert(sizeof(Word) == 8, "run_left reads the held uint2");
        int k;
        const int64_t wi = locate(i, j, &k);
        if (wi < 0) return 0;
        hold(wi);
        const uint64_t both = ((uint64_t)word.y << 32) | word.x;
        const uint64_t set = both & (0x0101010101010101ull * bit) & (~0ull >> (8 * (7 - k)));
        *opened = set != 0;
        return set ? k - (63 - __builtin_clzll(set)) / 8 + 1 : k + 1;
    }
};

// The same for K1gb: row after row in the band's frame, position b = j - i - lo of B, cells of BITS bits (4 or 8), cpl of them per lane
// that owns a position.  -1 outside rows 1..m, on column 0 and outside the band: a position below B lies inside its row's bytes.
template <int BITS>
struct BdCells {
    const uint8_t* ws = nullptr;
    int m, lo, B;
    int64_t rowbytes, nbytes;
    __host__ __device__ BdCells(int m_, int lo_, int B_, int cpl) : m(m_), lo(lo_), B(B_), rowbytes((int64_t)((B_ + cpl - 1) / cpl) * (cpl * BITS / 8)), nbytes(m_ * rowbytes) {}
    __host__ __device__ int64_t bytes() const { return nbytes; }
    __host__ __device__ int operator()(int i, int j) const
    {
        const uint32_t r = (uint32_t)(i - 1), b = (uint32_t)(j - i - lo);                         // unsigned: row 0 and a position below 0 wrap
        if (r >= (uint32_t)m || j < 1 || b >= (uint32_t)B) return -1;
        const int64_t bi = (int64_t)r * rowbytes + (BITS == 4 ? b >> 1 : b);
        return BITS == 4 ? (int)(((uint32_t)ws[bi] >> (4 * (b & 1))) & 15u) : (int)ws[bi];
    }
};

}  // namespace clh
