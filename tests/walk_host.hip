// walk_host.hip -- the walk-back of K1g and K1gb (pr_walk, EnCells, BdCells of csrc/ssw_pairs.h) on the CPU, over planes of random
// bytes.  Its control flow depends on memory contents and its contract is "whatever does not add up sets EN_ST_NO_WALK", so this
// program, built with AddressSanitizer and UBSan (tests/test_walk_host.py), feeds it what no score kernel stores: the plane is on
// the heap and exactly as large as the walk kernel's guard computes, `out` holds exactly cig_cap ops, and the sanitizers report a
// read outside either or a negative shift.  What the program itself asserts: a walk that is not refused leaves 0 <= nops <= cig_cap,
// begins inside [0, end], and ops whose lengths add up to the letters between begin and end (M on both sides, I on the query, D and N
// on the reference); and a gap state that reaches column 0 or row 0 is refused, in every model.  Nothing here touches a GPU.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "ssw_pairs.h"

using namespace clh;

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;                   // the fixed seed
static uint32_t rnd()
{
    g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
    return (uint32_t)(g_rng >> 24);
}
static int rnd_in(int lo, int hi) { return lo + (int)(rnd() % (uint32_t)(hi - lo + 1)); }

static long g_cases = 0, g_walked = 0, g_refused = 0, g_boundary = 0;

static void die(const char* what, const char* why, int m, int n, int mode, int ei, int ej)
{
    printf("walk_host: FAILED %s: %s (m %d, n %d, mode %d, end (%d, %d))\n", what, why, m, n, mode, ei, ej);
    exit(1);
}

// one walk from the end cell (ei, ej); true if it was not refused
template <int MODEL, typename Cells, typename Row0>
static bool walk_once(const char* what, Cells& cells, int m, int n, int mode, int ei, int ej, Row0 row0_op)
{
    const int cig_cap = std::min(m + n, 2 * std::min(m, n) + 1);
    uint32_t* out = new uint32_t[cig_cap];
    int32_t row[8] = {0, en_anchored(mode) ? 0 : -1, ej - 1, mode == EN_OVERLAP ? -1 : 0, ei - 1, 0, 0, 0};
    pr_walk<MODEL>(row, mode, m, n, out, cig_cap, cells, row0_op);
    const bool walked = row[7] != EN_ST_NO_WALK;
    if (walked) {
        const int nops = row[5], rb = row[1], qb = row[3];
        if (row[7] != 0) die(what, "a status that is neither 0 nor EN_ST_NO_WALK", m, n, mode, ei, ej);
        if (nops < 0 || nops > cig_cap) die(what, "nops outside [0, cig_cap]", m, n, mode, ei, ej);
        if (qb < 0 || qb > ei || rb < 0 || rb > ej) die(what, "a begin outside [0, end]", m, n, mode, ei, ej);
        long q = 0, r = 0;
        for (int k = 0; k < nops; ++k) {
            const int op = (int)(out[k] & 15u);
            const long len = (long)(out[k] >> 4);
            if (op > 3 || len < 1) die(what, "an op that is no M / I / D / N run", m, n, mode, ei, ej);
            if (k && op == (int)(out[k - 1] & 15u)) die(what, "two neighbouring runs of one op", m, n, mode, ei, ej);
            if (op == 0 || op == 1) q += len;
            if (op == 0 || op == 2 || op == 3) r += len;
        }
        if (q != ei - qb || r != ej - rb) die(what, "the ops do not add up to the letters between begin and end", m, n, mode, ei, ej);
    }
    delete[] out;
    return walked;
}

static uint8_t* random_plane(int64_t bytes)
{
    uint8_t* plane = new uint8_t[(size_t)bytes];                 // operator new aligns for every Word
    for (int64_t k = 0; k < bytes; ++k) plane[k] = (uint8_t)rnd();
    return plane;
}

// a plane in which every cell names the gap state `src` and no "opened here" is set: from (m, n) the walk runs into column 0 (a state
// that takes reference letters) or row 0 (one that takes query letters) in a gap state, which it must refuse
template <int MODEL, typename Cells, typename Row0>
static void boundary_case(const char* what, Cells cells, int m, int n, int src, Row0 row0_op)
{
    uint8_t* plane = new uint8_t[(size_t)cells.bytes()];
    memset(plane, MODEL == EN_ONE_PIECE ? src * 0x11 : src, (size_t)cells.bytes());
    cells.ws = (decltype(cells.ws))plane;
    if (walk_once<MODEL>(what, cells, m, n, EN_GLOBAL, m, n, row0_op)) die(what, "a gap state on the boundary was walked", m, n, EN_GLOBAL, m, n);
    delete[] plane;
    ++g_boundary;
}

template <int MODEL, typename Word, typename Row0>
static void run_ends(const char* what, int cases, Row0 row0_op)
{
    const long walked0 = g_walked;
    for (int c = 0; c < cases; ++c) {
        const bool wide = c % 16 == 15;                          // more than one chunk: the chunk term of the address
        const int m = rnd_in(1, 12), n = wide ? rnd_in(513, 530) : rnd_in(1, 12);
        EnCells<Word> cells(m, n);
        uint8_t* plane = random_plane(cells.bytes());
        cells.ws = (const Word*)plane;
        const int mode = rnd_in(EN_GLOBAL, EN_EXTEND);
        const int ei = rnd_in(0, m), ej = (wide && (rnd() & 1)) ? rnd_in(kEnChunk + 1, n) : rnd_in(0, n);
        const bool walked = walk_once<MODEL>(what, cells, m, n, mode, ei, ej, row0_op);
        ++g_cases; ++(walked ? g_walked : g_refused);
        delete[] plane;
    }
    if (g_walked == walked0) die(what, "no case was walked", 0, 0, 0, 0, 0);
    constexpr int ref_gap = 1, qry_gap = MODEL == EN_ONE_PIECE ? 2 : 3;      // E (E_1) and F (F_1)
    for (int n : {5, 520}) {
        EnCells<Word> cells(7, n);
        boundary_case<MODEL>(what, cells, 7, n, ref_gap, row0_op);
        boundary_case<MODEL>(what, cells, 7, n, qry_gap, row0_op);
    }
}

template <int MODEL, int BITS>
static void run_band(const char* what, int cases)
{
    const long walked0 = g_walked;
    for (int c = 0; c < cases; ++c) {
        const int m = rnd_in(1, 12), n = rnd_in(1, 12);
        const int cls = c % kBdClasses, cpl = kBdCpl[cls];       // bands of every class
        const int lo = rnd_in(-m, n), hi = rnd_in(lo, n);
        BdCells<BITS> cells(m, lo, hi - lo + 1, cpl);
        uint8_t* plane = random_plane(cells.bytes());
        cells.ws = plane;
        const int modes[4] = {EN_GLOBAL, EN_SEMIGLOBAL, EN_PREFIX, EN_EXTEND};
        const int mode = modes[rnd() & 3];
        const int ei = rnd_in(0, m), ej = rnd_in(0, n);
        const bool walked = walk_once<MODEL>(what, cells, m, n, mode, ei, ej, PrRow0D());
        ++g_cases; ++(walked ? g_walked : g_refused);
        delete[] plane;
    }
    if (g_walked == walked0) die(what, "no case was walked", 0, 0, 0, 0, 0);
    constexpr int ref_gap = 1, qry_gap = MODEL == EN_ONE_PIECE ? 2 : 3;
    for (int cls = 0; cls < kBdClasses; ++cls) {
        BdCells<BITS> cells(7, -7, 5 + 7 + 1, kBdCpl[cls]);      // the whole matrix of 7 x 5
        boundary_case<MODEL>(what, cells, 7, 5, ref_gap, PrRow0D());
        boundary_case<MODEL>(what, cells, 7, 5, qry_gap, PrRow0D());
    }
}

int main()
{
    const int cases = 20000;
    run_ends<EN_ONE_PIECE, uint32_t>("K1g one piece", cases, PrRow0D());
    run_ends<EN_TWO_PIECE, uint8_t>("K1g two pieces", cases, PrRow0D());
    run_ends<EN_SPLICED, uint2>("K1g spliced", cases, [](int j) -> int { return (j & 1) ? 2 : 3; });
    run_band<EN_ONE_PIECE, 4>("K1gb one piece", cases);
    run_band<EN_TWO_PIECE, 8>("K1gb two pieces", cases);
    printf("walk_host: 5 instantiations, %ld cases, %ld walked, %ld refused, %ld boundary cases refused: ok\n", g_cases, g_walked, g_refused, g_boundary);
    return 0;
}
