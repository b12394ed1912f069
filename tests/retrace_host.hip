// retrace_host.hip -- the resumable walk of K1g's recompute route (pr_walk_round, EnTile, EnKept of csrc/ssw_pairs.h) on the CPU, held to
// pr_walk over EnCells on the same decisions: the two are one body (pr_walk_steps), tiled with a record between rounds and untiled.  For random (m, n) of one to five chunks and each gap model a whole plane is drawn --
// random bytes, or mostly cells that name a reference-gap state, so that runs cross whole chunks -- and walked once by pr_walk.  Then
// the record a keeping score pass would leave is walked round after round: each round's tile is a heap buffer of exactly the bytes
// EnKept gives one chunk's plane, filled with that chunk's words of the plane for the rows up to the record's row limit and with
// other random bytes above them.  Row fields, ops and the EN_ST_NO_WALK verdict must be those of pr_walk.  Some records are damaged
// between rounds: such a walk may end either way, but inside its buffers.  Built with AddressSanitizer and UBSan
// (tests/test_retrace_walk_host.py); nothing here touches a GPU.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "ssw_pairs.h"

using namespace clh;

static uint64_t g_rng = 0x2545f4914f6cdd1dull;                   // the fixed seed
static uint32_t rnd()
{
    g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
    return (uint32_t)(g_rng >> 24);
}
static int rnd_in(int lo, int hi) { return lo + (int)(rnd() % (uint32_t)(hi - lo + 1)); }

static long g_cases = 0, g_walked = 0, g_refused = 0, g_resumed = 0, g_damaged = 0;

static void die(const char* what, const char* why, int m, int n, int mode, int ei, int ej)
{
    printf("retrace_host: FAILED %s: %s (m %d, n %d, mode %d, end (%d, %d))\n", what, why, m, n, mode, ei, ej);
    exit(1);
}

// a plane of `bytes` bytes whose cells (half-bytes for one piece, bytes otherwise) are random, or, with `runs`, mostly a reference-gap state
// without its "opened here": the walk then runs leftwards through chunk after chunk
template <int MODEL>
static uint8_t* draw_plane(int64_t bytes, bool runs)
{
    uint8_t* plane = new uint8_t[(size_t)bytes];
    for (int64_t k = 0; k < bytes; ++k) {
        uint8_t b = (uint8_t)rnd();
        if (runs && (rnd() & 63)) {
            const uint8_t s = (uint8_t)(MODEL == EN_ONE_PIECE ? 1 : 1 + (k >> 9 & 1));
            b = MODEL == EN_ONE_PIECE ? (uint8_t)(s * 0x11) : s;
        }
        plane[k] = b;
    }
    return plane;
}

template <int MODEL, typename Word, typename Row0>
static void run_model(const char* what, int cases, int nh, Row0 row0_op)
{
    constexpr int word_bytes = sizeof(Word) == 4 ? 4 : 8;
    const long resumed0 = g_resumed, walked0 = g_walked;
    for (int t = 0; t < cases; ++t) {
        const int m = rnd_in(1, 40), nchunks = rnd_in(1, 5);
        const int n = (nchunks - 1) * kEnChunk + (t % 5 == 0 ? kEnChunk : rnd_in(1, kEnChunk));
        const int mode = rnd_in(EN_GLOBAL, EN_EXTEND);
        const int ei = t % 7 == 0 ? rnd_in(0, m) : m, ej = t % 3 == 0 ? rnd_in(0, n) : n;
        const int cig_cap = std::min(m + n, 2 * std::min(m, n) + 1);
        EnCells<Word> cells(m, n);
        uint8_t* plane = draw_plane<MODEL>(cells.bytes(), t % 4 != 0);
        cells.ws = (const Word*)plane;
        // the stored route
        uint32_t* out_a = new uint32_t[cig_cap];
        int32_t row_a[8] = {0, en_anchored(mode) ? 0 : -1, ej - 1, mode == EN_OVERLAP ? -1 : 0, ei - 1, 0, 0, 0};
        pr_walk<MODEL>(row_a, mode, m, n, out_a, cig_cap, cells, row0_op);
        // the recompute route: the record of the keeping pass, then a tile and a round of the walk per chunk
        const EnKept lay(m, n, nh, word_bytes);
        const int64_t tile_bytes = lay.rec_off - lay.plane_off;
        if (tile_bytes != (int64_t)word_bytes * m * 64 || lay.plane_off != (int64_t)4 * nh * ((m + 63) & ~63) * (nchunks - 1) || (lay.total & 15) ||
            lay.total < lay.rec_off + 4 * kEnRecWords) die(what, "EnKept is not the layout the header states", m, n, mode, ei, ej);
        uint32_t* out_b = new uint32_t[cig_cap];
        int32_t row_b[8] = {0, en_anchored(mode) ? 0 : -1, ej - 1, mode == EN_OVERLAP ? -1 : 0, ei - 1, 0, 0, 0};
        int32_t rec[kEnRecWords] = {0};
        rec[EN_REC_DONE] = 0; rec[EN_REC_CHUNK] = ej > 0 ? (ej - 1) / kEnChunk : 0; rec[EN_REC_I] = ei; rec[EN_REC_J] = ej;
        rec[EN_REC_STATE] = 0; rec[EN_REC_CUR] = -1; rec[EN_REC_RUN] = 0; rec[EN_REC_NOPS] = 0; rec[EN_REC_STEPS] = ei + ej + 2;
        bool damaged = false;
        int rounds = 0;
        for (int r = 0; r < nchunks && row_b[7] == 0 && rec[EN_REC_DONE] == 0; ++r, ++rounds) {
            int c = rec[EN_REC_CHUNK], ilim = rec[EN_REC_I];
            c = c < 0 ? 0 : (c > nchunks - 1 ? nchunks - 1 : c);             // as the tile form and the walk kernel clamp them
            ilim = ilim > m ? m : (ilim < 0 ? 0 : ilim);
            uint8_t* tile = new uint8_t[(size_t)tile_bytes];
            for (int64_t k = 0; k < tile_bytes; ++k) tile[k] = (uint8_t)rnd();
            EnTile<Word> tc(m, n, c, ilim);
            const int64_t chunk_words = (int64_t)c * m * 64;                     // where EnCells has chunk c
            memcpy(tile, plane + chunk_words * word_bytes, (size_t)ilim * tc.L * word_bytes);
            tc.ws = (const Word*)tile;
            pr_walk_round<MODEL>(rec, row_b, mode, m, n, out_b, cig_cap, tc, c, r == nchunks - 1, row0_op);
            delete[] tile;
            if (rec[EN_REC_DONE] == 0 && t % 16 == 5 && !damaged) {             // damage one field of a suspended record
                rec[rnd_in(EN_REC_CHUNK, EN_REC_STEPS)] = (int32_t)rnd() - (1 << 20) * (int)(rnd() & 1);
                damaged = true; ++g_damaged;
            }
        }
        if (rounds > 1) ++g_resumed;
        if (!damaged) {
            if (rec[EN_REC_DONE] == 0 && row_b[7] == 0) die(what, "a pair is still open after nchunks rounds", m, n, mode, ei, ej);
            if ((row_a[7] == EN_ST_NO_WALK) != (row_b[7] == EN_ST_NO_WALK)) die(what, "the two walks disagree on EN_ST_NO_WALK", m, n, mode, ei, ej);
            if (row_a[7] != EN_ST_NO_WALK) {
                if (memcmp(row_a, row_b, sizeof row_a)) die(what, "the rows differ", m, n, mode, ei, ej);
                if (row_a[5] < 0 || row_a[5] > cig_cap || memcmp(out_a, out_b, sizeof(uint32_t) * (size_t)row_a[5])) die(what, "the ops differ", m, n, mode, ei, ej);
            }
        } else if (row_b[7] == 0 && rec[EN_REC_DONE] != 0 && (row_b[5] < 0 || row_b[5] > cig_cap)) die(what, "a damaged record left nops outside [0, cig_cap]", m, n, mode, ei, ej);
        ++g_cases; ++(row_a[7] == EN_ST_NO_WALK ? g_refused : g_walked);
        delete[] out_a; delete[] out_b; delete[] plane;
    }
    if (g_resumed == resumed0) die(what, "no walk was resumed", 0, 0, 0, 0, 0);
    if (g_walked == walked0) die(what, "no case was walked", 0, 0, 0, 0, 0);
}

int main()
{
    const int cases = 6000;
    run_model<EN_ONE_PIECE, uint32_t>("one piece", cases, 2, PrRow0D());
    run_model<EN_TWO_PIECE, uint8_t>("two pieces", cases, 3, PrRow0D());
    run_model<EN_SPLICED, uint2>("spliced", cases, 3, [](int j) -> int { return (j & 1) ? 2 : 3; });
    printf("retrace_host: 3 models, %ld cases, %ld walked, %ld refused, %ld resumed, %ld records damaged: ok\n", g_cases, g_walked, g_refused, g_resumed, g_damaged);
    return 0;
}
