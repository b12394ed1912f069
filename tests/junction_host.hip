// junction_host.hip -- the __host__ __device__ helpers of K7j (csrc/seed_device.h: jx_status, jx_class, jx_nd, jx_na, jx_letter, jx_site,
// jx_read_letter) on the CPU, under AddressSanitizer and UBSan.  A program of its own: it prints its inputs and answers, one case a
// line, at every clip, contig-end, code-4 and strand case, and tests/test_junction_host.py compares every line with
// tests/junction_check.py.  No GPU is touched.
#include <stdio.h>
#include <stdint.h>
#include <vector>
#include "seed_device.h"

using namespace clh;

int main()
{
    int lines = 0;
    // three contigs side by side, exactly as long as the allocation: the first ends with AG, the third begins with GT, bytes with
    // the case and N bits set above the code and with codes 5..7 (read as 4)
    const char* text[3] = {"ACGTTGCAAG", "GTACNGTAGCTAGGTnACAG", "GTCCA"};
    std::vector<uint8_t> genome;
    int64_t off[3], len[3];
    for (int c = 0; c < 3; ++c) {
        off[c] = (int64_t)genome.size();
        for (const char* p = text[c]; *p; ++p) {
            const int i = (int)genome.size();
            int code = *p == 'A' ? 0 : *p == 'C' ? 1 : *p == 'G' ? 2 : *p == 'T' ? 3 : *p == 'n' ? 5 + i % 3 : 4;
            genome.push_back((uint8_t)(code | ((i * 7) % 32) << 3));
        }
        len[c] = (int64_t)genome.size() - off[c];
    }
    int32_t site[kJxSites];
    for (int i = 0; i < kJxSites; ++i) site[i] = 100 + i;          // every entry its own cost: the line names the entry that was read
    for (int c = 0; c < 3; ++c) {
        printf("contig %d", c);
        for (int64_t x = 0; x < len[c]; ++x) printf(" %d", (int)genome[(size_t)(off[c] + x)]);
        printf("\n"); ++lines;
        for (int64_t x = -3; x <= len[c] + 2; ++x) { printf("letter %d %lld %d\n", c, (long long)x, jx_letter(genome.data(), off[c], len[c], x)); ++lines; }
        for (int64_t p = -3; p <= len[c] + 1; ++p)
            for (int part = 0; part < 2; ++part)
                for (int minus = 0; minus < 2; ++minus) {
                    printf("site %d %lld %d %d %d\n", c, (long long)p, part, minus, jx_site(site, genome.data(), off[c], len[c], p, part, minus) - 100); ++lines;
                }
    }
    const int8_t read[7] = {0, 1, 2, 3, 4, 3, 1};
    for (int minus = 0; minus < 2; ++minus)
        for (int64_t y = -1; y <= 7; ++y) { printf("read %d %lld %d\n", minus, (long long)y, jx_read_letter(read, 7, y, minus)); ++lines; }
    const int64_t ms[] = {0, 1, 5, 64, 512}, slacks[] = {0, 16, 64}, lens[] = {0, 1, 30, 600, 4000};
    for (int64_t L : lens)
        for (int64_t m : ms)
            for (int64_t s : slacks)
                for (int64_t x : {(int64_t)0, (int64_t)1, L / 2, L - 1, L})
                    if (x >= 0 && x <= L) { printf("clip %lld %lld %lld %lld %lld %lld\n", (long long)x, (long long)m, (long long)s, (long long)L,
                                                   (long long)jx_nd(x, m, s, L), (long long)jx_na(x, m, s)); ++lines; }
    for (int64_t xd : {0, 5, 6})
        for (int64_t xa : {0, 5, 6})
            for (int64_t m : {-1, 0, 1, 2, 64, 65, 128, 129, 256, 257, 511, 512, 513})
                for (int64_t span : {1, 64, 512}) {
                    printf("status %lld %lld %lld %lld %lld %d %d\n", (long long)xd, (long long)10, (long long)xa, (long long)(10 + m), (long long)span,
                           jx_status(xd, 10, xa, 10 + m, span), m >= 1 ? jx_class(m) : -1); ++lines;
                }
    printf("junction_host: %d lines: ok\n", lines);
    return 0;
}
