// ssw_pairs.h -- what K1g (ssw_ends.hip) and K1gb (ssw_band.hip) share on the device: the LDS matrix of their score kernels and the
// walks back over the stored decisions, one per gap model: pr_walk (one piece), pr_walk2 (two pieces, both kernels), pr_walk_spliced
// (intron gaps, K1g alone).  The two kernels differ in where a cell's decisions lie, which a walk takes as a functor.
// (Each of the two score kernels is one template body for all its gap models.  The decision bits of a cell and the end cell's argmax
// over the wave are the same text in both and stay written out there: as helpers they changed the register allocation of the storing
// forms -- LABNOTES.md 16 and 20 have the tables.)
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

// One lane walks one pair's stored decisions back from the end cell its score kernel left in `row` (tie rules: diagonal, then E,
// then F; a gap is left as soon as "opened here" is set), writes the CIGAR (BAM ops M 0, I 1, D 2) and the begins; at most
// i + j + 2 steps.  cell(i, j) gives the 4 bits of cell (i, j), or -1 where the cell is outside what was stored.  Whatever
// does not add up sets EN_ST_NO_WALK, which fetch reports.  The caller has checked the pair's own geometry and that `out` holds cig_cap ops.
template <typename Cell>
__device__ __forceinline__ void pr_walk(int32_t* row, int mode, int m, int n, uint32_t* out, int cig_cap, Cell cell)
{
    int i = row[4] + 1, j = row[2] + 1;
    if (i < 0 || i > m || j < 0 || j > n) { row[7] = EN_ST_NO_WALK; return; }
    const int steps = i + j + 2;
    int state = 0, nops = 0, cur = -1, run = 0;
    bool bad = false, done = false;
    auto emit = [&](int op, int k) {
        if (k <= 0) return;
        if (op == cur) { run += k; return; }
        if (run) { if (nops < cig_cap) out[nops++] = ((uint32_t)run << 4) | (uint32_t)cur; else bad = true; }
        cur = op; run = k;
    };
    for (int step = 0; step < steps && !done; ++step) {
        if (state == 0 && (i == 0 || j == 0)) {
            if (en_anchored(mode)) { emit(2, j); emit(1, i); i = 0; j = 0; }      // prefix and extend stop at (0, 0) as global does
            else if (mode == EN_SEMIGLOBAL && j == 0) { emit(1, i); i = 0; }
            done = true;
            break;
        }
        const int at = cell(i, j);
        if (at < 0) { bad = true; break; }
        const uint32_t nib = (uint32_t)at;
        if (state == 0) {
            state = (int)(nib & 3u);                             // a gap state takes its first letter from this same cell
            if (state == 0) { emit(0, 1); --i; --j; continue; }
        }
        if (state == 1) { emit(2, 1); --j; if (nib & 4u) state = 0; }
        else if (state == 2) { emit(1, 1); --i; if (nib & 8u) state = 0; }
        else { bad = true; break; }
    }
    emit(-2, 1);                                                 // flush the last run
    if (bad || !done) { row[7] = EN_ST_NO_WALK; return; }
    for (int a = 0, b = nops - 1; a < b; ++a, --b) { const uint32_t w = out[a]; out[a] = out[b]; out[b] = w; }
    row[1] = j; row[3] = i; row[5] = nops;
}

// pr_walk for two-piece gap costs (ssw_ends.hip, ssw_band.hip).  cell(i, j) gives the byte of cell (i, j) -- bits 0..2 H's source (0 diagonal, 1 E_1,
// 2 E_2, 3 F_1, 4 F_2: that order is the tie rule), bits 3..6 "opened here" of E_1, E_2, F_1, F_2 -- or -1 outside what was stored.  Both
// pieces of a direction emit the same op; a gap state is left as soon as its own piece's "opened here" is set.  Steps, bounds and
// EN_ST_NO_WALK as in pr_walk.
template <typename Cell>
__device__ __forceinline__ void pr_walk2(int32_t* row, int mode, int m, int n, uint32_t* out, int cig_cap, Cell cell)
{
    int i = row[4] + 1, j = row[2] + 1;
    if (i < 0 || i > m || j < 0 || j > n) { row[7] = EN_ST_NO_WALK; return; }
    const int steps = i + j + 2;
    int state = 0, nops = 0, cur = -1, run = 0;
    bool bad = false, done = false;
    auto emit = [&](int op, int k) {
        if (k <= 0) return;
        if (op == cur) { run += k; return; }
        if (run) { if (nops < cig_cap) out[nops++] = ((uint32_t)run << 4) | (uint32_t)cur; else bad = true; }
        cur = op; run = k;
    };
    for (int step = 0; step < steps && !done; ++step) {
        if (state == 0 && (i == 0 || j == 0)) {
            if (en_anchored(mode)) { emit(2, j); emit(1, i); i = 0; j = 0; }
            else if (mode == EN_SEMIGLOBAL && j == 0) { emit(1, i); i = 0; }
            done = true;
            break;
        }
        const int at = cell(i, j);
        if (at < 0) { bad = true; break; }
        const uint32_t b = (uint32_t)at;
        if (state == 0) {
            state = (int)(b & 7u);                               // a gap state takes its first letter from this same cell
            if (state == 0) { emit(0, 1); --i; --j; continue; }
        }
        if (state == 1 || state == 2) { emit(2, 1); --j; if (b & (4u << state)) state = 0; }          // bit 3 for E_1, bit 4 for E_2
        else if (state == 3 || state == 4) { emit(1, 1); --i; if (b & (4u << state)) state = 0; }     // bit 5 for F_1, bit 6 for F_2
        else { bad = true; break; }
    }
    emit(-2, 1);                                                 // flush the last run
    if (bad || !done) { row[7] = EN_ST_NO_WALK; return; }
    for (int a = 0, c = nops - 1; a < c; ++a, --c) { const uint32_t w = out[a]; out[a] = out[c]; out[c] = w; }
    row[1] = j; row[3] = i; row[5] = nops;
}

// pr_walk for spliced alignment (ssw_ends.hip).  cell(i, j) gives the byte of cell (i, j) -- bits 0..1 H's source (0 diagonal, 1 E, 2 N,
// 3 F: that order is the tie rule), bit 2 T's source (0 diagonal, 1 F), bits 3..5 "opened here" of E, N, F -- or -1 outside what was
// stored.  E emits D (2), N emits N (3); on leaving either the walk is in state T (4), H without a reference gap: the diagonal if T
// equals it, else F, never E or N again, so that no D stands next to an N.  row0_op(j) names the op of the one run of j letters the
// anchored stop on row 0 emits.  run(i, j, bit, &opened) gives how many cells of the E or N run that stands on (i, j) lie in the
// stored word of that cell, from column j leftwards up to and including the first whose `bit` ("opened here") is set, or 0 outside what
// was stored: an intron is thousands of cells along one row, taken 8 at a step.  Every step consumes a letter; steps, bounds and
// EN_ST_NO_WALK as in pr_walk.
template <typename Cell, typename Run, typename Row0>
__device__ __forceinline__ void pr_walk_spliced(int32_t* row, int mode, int m, int n, uint32_t* out, int cig_cap, Cell cell, Run run_left, Row0 row0_op)
{
    int i = row[4] + 1, j = row[2] + 1;
    if (i < 0 || i > m || j < 0 || j > n) { row[7] = EN_ST_NO_WALK; return; }
    const int steps = i + j + 2;
    int state = 0, nops = 0, cur = -1, run = 0;
    bool bad = false, done = false;
    auto emit = [&](int op, int k) {
        if (k <= 0) return;
        if (op == cur) { run += k; return; }
        if (run) { if (nops < cig_cap) out[nops++] = ((uint32_t)run << 4) | (uint32_t)cur; else bad = true; }
        cur = op; run = k;
    };
    for (int step = 0; step < steps && !done; ++step) {
        if ((state == 0 || state == 4) && (i == 0 || j == 0)) {      // on column 0 T is H; state T never stands on row 0
            if (en_anchored(mode)) { if (j > 0) emit(row0_op(j), j); emit(1, i); i = 0; j = 0; }
            else if (mode == EN_SEMIGLOBAL && j == 0) { emit(1, i); i = 0; }
            done = true;
            break;
        }
        if (i <= 0 || j <= 0) { bad = true; break; }              // a gap state on the boundary: the stored bits do not add up
        const int at = cell(i, j);
        if (at < 0) { bad = true; break; }
        const uint32_t b = (uint32_t)at;
        if (state == 0) {
            state = (int)(b & 3u);                               // a gap state takes its first letter from this same cell
            if (state == 0) { emit(0, 1); --i; --j; continue; }
        } else if (state == 4) {
            if (!(b & 4u)) { emit(0, 1); --i; --j; state = 0; continue; }
            state = 3;
        }
        if (state == 1 || state == 2) {
            bool opened = false;
            const int k = run_left(i, j, state == 1 ? 8u : 16u, &opened);
            if (k <= 0 || k > j) { bad = true; break; }
            emit(state == 1 ? 2 : 3, k); j -= k;
            if (opened) state = 4;
        }
        else { emit(1, 1); --i; if (b & 32u) state = 0; }
    }
    emit(-2, 1);                                                 // flush the last run
    if (bad || !done) { row[7] = EN_ST_NO_WALK; return; }
    for (int a = 0, c = nops - 1; a < c; ++a, --c) { const uint32_t w = out[a]; out[a] = out[c]; out[c] = w; }
    row[1] = j; row[3] = i; row[5] = nops;
}

}  // namespace clh
