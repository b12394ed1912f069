// seed_host.hip -- the __host__ __device__ functions of csrc/seed_device.h on the CPU, under AddressSanitizer and UBSan: the packing and
// the mix (sd_roll_push, sd_roll_key, sd_mix), the selection rule for one position (sd_selected) over key arrays exactly as long as the
// sequence has positions, and the chain transition (ch_gain).  A program of its own: it prints its inputs and its answers for a fixed
// seeded case list and tests/test_seed_host.py compares every line with tests/seed_check.py.  No GPU is touched.
#include <stdint.h>
#include <stdio.h>
#include <vector>
#include "seed_device.h"

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd()
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return g_state >> 33;
}

int main()
{
    using namespace clh;
    int lines = 0;
    const int ks[3] = {4, 15, 28};
    for (int k : ks) {
        const uint64_t m = ((uint64_t)1 << (2 * k)) - 1;
        for (int t = 0; t < 60; ++t) {
            const uint64_t h = t < 4 ? (t & 1 ? m - t / 2 : (uint64_t)(t / 2)) : ((rnd() << 31) ^ rnd()) & m;
            printf("mix %d %llu %llu\n", k, (unsigned long long)h, (unsigned long long)sd_mix(h, m));
            ++lines;
        }
    }
    for (int c = 0; c < 240; ++c) {
        const int k = 4 + (int)(rnd() % 6), w = 1 + (int)(rnd() % 8), alpha = c % 3 == 0 ? 2 : (c % 3 == 1 ? 4 : 5), n = (int)(rnd() % 81);
        std::vector<uint8_t> seq((size_t)n);
        for (auto& b : seq) b = (uint8_t)((rnd() % alpha) | (rnd() % 4 == 0 ? 8 : 0));      // bit 3 (soft mask) set here and there: ignored
        printf("seq %d %d %d ", c, k, w);
        for (uint8_t b : seq) putchar('0' + (b & 7));
        putchar('\n');
        ++lines;
        const int P = n - k + 1;
        if (P <= 0) continue;
        const uint64_t m = ((uint64_t)1 << (2 * k)) - 1;
        std::vector<uint64_t> v((size_t)P);
        SdRoll roll;
        sd_roll_init(&roll);
        for (int t = 0; t < n; ++t) {
            sd_roll_push(&roll, seq[t], k, m);
            if (t >= k - 1) v[t - k + 1] = sd_roll_key(roll, k, m);
        }
        const int wp = w < P ? w : P;
        for (int p = 0; p < P; ++p) {
            // as a kernel holds them: the positions within wp - 1 of p only, in an array of exactly that length
            const int lo = p - (wp - 1) > 0 ? p - (wp - 1) : 0, hi = p + wp < P ? p + wp : P;
            std::vector<uint64_t> part(v.begin() + lo, v.begin() + hi);
            const bool sel = sd_selected(part.data(), lo, hi, p, wp);
            if (sel != sd_selected(v.data(), 0, P, p, wp)) { printf("seed_host: position %d of case %d differs between the part and the whole\n", p, c); return 1; }
            if (sel) { printf("min %d %d %llu %d\n", c, p, (unsigned long long)(v[p] >> 1), (int)(v[p] & 1)); ++lines; }
        }
    }
    for (int t = 0; t < 400; ++t) {
        const int k = 4 + (int)(rnd() % 25);
        const long long dx = 1 + (long long)(rnd() % (t < 200 ? 40 : 6000)), dy = t % 5 == 0 ? dx : 1 + (long long)(rnd() % (t < 200 ? 40 : 6000));
        printf("gain %lld %lld %d %lld\n", dx, dy, k, (long long)ch_gain(dx, dy, k));
        ++lines;
    }
    printf("seed_host: %d lines: ok\n", lines);
    return 0;
}
