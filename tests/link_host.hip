// link_host.hip -- the __host__ __device__ link functions of csrc/seed_device.h (lk_before, lk_link: the very code seed_link_kernel runs)
// on the CPU, under AddressSanitizer and UBSan.  A program of its own: it prints its inputs and its answers for a fixed seeded case list
// and tests/test_link_host.py compares every line with tests/link_check.py.  The cases sit on and beside every threshold, and at the
// limits of what the C ABI lets through (coordinates up to 2^40 - 1, costs up to 2^40 - 1, bounds up to INT64_MAX).  No GPU is touched.
#include <stdint.h>
#include <stdio.h>
#include "seed_device.h"

static uint64_t g_state = 0x2545f4914f6cdd1dull;
static uint64_t rnd()
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return g_state >> 33;
}
static int64_t pick(int64_t lo, int64_t hi) { return lo + (int64_t)(rnd() % (uint64_t)(hi - lo + 1)); }

static void show(const clh::LkChain& c) { printf(" %lld %lld %lld %lld %lld %lld", (long long)c.g, (long long)c.score, (long long)c.x0, (long long)c.x1, (long long)c.y0, (long long)c.y1); }

static int emit(const clh::LkChain& j, const clh::LkChain& i, const clh::LkParams& p, int k)
{
    int kind = -1;
    const int64_t term = clh::lk_link(j, i, p, k, &kind);
    if ((term == clh::kLkNone) != (kind == 0) || (term != clh::kLkNone && term > 0)) { printf("link_host: a link of kind %d with term %lld\n", kind, (long long)term); return 1; }
    printf("link %d %lld %lld %lld %lld %lld %lld %lld", k, (long long)p.max_query_gap, (long long)p.max_overlap, (long long)p.max_skew, (long long)p.max_intron,
           (long long)p.max_circle, (long long)p.intron_cost, (long long)p.backsplice_cost);
    show(j); show(i);
    if (term == clh::kLkNone) printf(" %d none\n", kind); else printf(" %d %lld\n", kind, (long long)term);
    return 0;
}

int main()
{
    using namespace clh;
    int lines = 0;
    const int64_t top = kLkLimit - 1, big = INT64_MAX;
    // on and beside every threshold: j ends at (x 10000, y 1000), i starts q letters on in the read and d further on the contig
    const LkParams base = {500, 32, 500, 200000, 200000, 16, 32};
    const int64_t qs[8] = {0, 1, 500, 501, -1, -32, -33, 250};
    const int64_t ds[14] = {0, 1, -1, 500, 501, -500, -501, 200000, 200001, -200000, -9000, -9499, -9500, -9501};
    for (int64_t q : qs)
        for (int64_t d : ds)
            for (int len = 0; len < 2; ++len) {
                const LkChain j = {0, 100, 9000, 10000, 0, 1000};
                const int64_t x0 = 10000 + q + d, y0 = 1000 + q, n = len ? 700 : 40;
                if (x0 < 0) continue;
                const LkChain i = {0, 80, x0, x0 + n, y0, y0 + n};
                if (emit(j, i, base, 15)) return 1;
                ++lines;
            }
    // the circle's span on its own: the back-splice target starts `span` below the source's end
    for (int64_t span : {(int64_t)-1, (int64_t)0, (int64_t)1, (int64_t)2, (int64_t)699, (int64_t)700, (int64_t)701})
        for (int64_t mc : {(int64_t)0, (int64_t)1, (int64_t)700, big}) {
            LkParams p = base;
            p.max_circle = mc; p.max_skew = 0;
            const LkChain j = {3, 50, 5000, 6000, 100, 200}, i = {3, 50, 6000 - span, 6000 - span + 90, 210, 300};
            if (emit(j, i, p, 15)) return 1;
            ++lines;
        }
    // order, contig and the limits of the interface
    {
        const LkChain a = {1, 40, top - 100, top, top - 100, top}, b = {1, 40, 0, 100, 0, 100}, c = {2, 40, 0, 100, 0, 100};
        const LkParams wide = {big, big, 0, big, big, top, top}, all = {big, big, big, big, big, 0, 0};
        for (const LkParams& p : {wide, all, base}) {
            const LkChain* v[3] = {&a, &b, &c};
            for (int s = 0; s < 3; ++s)
                for (int t = 0; t < 3; ++t) {
                    if (emit(*v[s], *v[t], p, 28)) return 1;
                    ++lines;
                }
        }
    }
    for (int t = 0; t < 3000; ++t) {
        const int k = 4 + (int)(rnd() % 25);
        const bool small = t % 3 != 0;
        LkParams p;
        p.max_query_gap = pick(0, small ? 8 : 600); p.max_overlap = pick(0, small ? 4 : 40); p.max_skew = pick(0, small ? 6 : 600);
        p.max_intron = p.max_skew + pick(0, small ? 10 : 300000); p.max_circle = pick(0, small ? 12 : 300000);
        p.intron_cost = pick(0, 40); p.backsplice_cost = pick(0, 40);
        const int64_t span = small ? 24 : 400000;
        LkChain c[2];
        for (LkChain& v : c) {
            v.g = pick(0, t % 7 == 0 ? 1 : 0); v.score = pick(-5, 300);
            v.x0 = pick(0, span); v.x1 = v.x0 + pick(1, small ? 8 : 2000); v.y0 = pick(0, small ? 16 : 3000); v.y1 = v.y0 + pick(1, small ? 8 : 2000);
        }
        if (t % 2 == 0) {                              // i placed behind j, around every bound
            const int64_t q = pick(-(p.max_overlap + 2), p.max_query_gap + 2), d = pick(-(p.max_circle + p.max_skew + 5), p.max_intron + 5);
            const int64_t y0 = c[0].y1 + q, x0 = c[0].x1 + q + d;
            c[1].g = c[0].g; c[1].y0 = y0 < 0 ? 0 : y0; c[1].y1 = c[1].y0 + pick(1, 300); c[1].x0 = x0 < 0 ? 0 : x0; c[1].x1 = c[1].x0 + pick(1, 300);
        }
        if (emit(c[0], c[1], p, k)) return 1;
        ++lines;
        printf("before");
        show(c[0]); printf(" %d", (int)(t % 5)); show(c[1]); printf(" %d", (int)(t % 4));
        printf(" %d\n", lk_before(c[0], t % 5, c[1], t % 4) ? 1 : 0);
        ++lines;
    }
    for (int t = 0; t < 400; ++t) {                    // the order on its ties: fields drawn from two values
        LkChain c[2];
        for (LkChain& v : c) { v.g = 0; v.score = 1; v.x0 = pick(0, 1); v.x1 = 9; v.y0 = pick(0, 1); v.y1 = pick(2, 3); }
        const int ca = (int)pick(0, 2), cb = (int)pick(0, 2);
        printf("before");
        show(c[0]); printf(" %d", ca); show(c[1]); printf(" %d", cb);
        printf(" %d\n", lk_before(c[0], ca, c[1], cb) ? 1 : 0);
        ++lines;
    }
    printf("link_host: %d lines: ok\n", lines);
    return 0;
}
