// circle_host.hip -- the __host__ __device__ selection functions of csrc/seed_device.h on the CPU, under AddressSanitizer and UBSan:
// cc_tie_key, cc_path_before, cc_task, cc_task_ok, cc_ordinal, cc_winner, cc_flanks and cc_read_pos, which the kernels of
// seed_circle.hip call, and cc_best_path, the serial statement of the selection that no kernel runs (the select kernel reduces with the
// same cc_tie_key and cc_path_before per lane and across the wave; that reduction is covered by tests/test_gpu_circles.py alone).
// A program of its own: it reads the planted segments that tests/test_circle_host.py wrote (chain rows, link rows and K7j rows of the
// checkers) from the file named on its command line, prints per read the path it selects, its tasks and
// its circle row, and the test compares every line with tests/circle_check.py.  No GPU is touched.
//
// The file, all integers, blank-separated:  k  min_path_score  max_span  contigs;  per contig: its length, its resident bytes;  reads;
// per read: L, the chains of its plus and minus segment n0 n1, then n0 + n1 chain rows of 10 words and as many link rows of 8 words,
// then the number of K7j rows the checker made for its tasks and those rows of 12 words.
#include <stdint.h>
#include <stdio.h>
#include <vector>
#include "seed_device.h"

static bool next(FILE* f, int64_t* v)
{
    long long x = 0;
    if (fscanf(f, "%lld", &x) != 1) return false;
    *v = x;
    return true;
}

int main(int argc, char** argv)
{
    using namespace clh;
    if (argc != 2) { fprintf(stderr, "usage: circle_host FILE\n"); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "circle_host: cannot open %s\n", argv[1]); return 2; }
    int64_t k = 0, min_path_score = 0, max_span = 0, n_contigs = 0, n_reads = 0, v = 0;
    if (!next(f, &k) || !next(f, &min_path_score) || !next(f, &max_span) || !next(f, &n_contigs) || n_contigs < 0 || n_contigs > 64) return 3;
    std::vector<uint8_t> genome;
    std::vector<int64_t> off, len;
    for (int64_t c = 0; c < n_contigs; ++c) {
        if (!next(f, &v) || v < 0 || v > 8192) return 3;
        off.push_back((int64_t)genome.size()); len.push_back(v);
        for (int64_t i = 0; i < len.back(); ++i) {
            if (!next(f, &v) || v < 0 || v > 255) return 3;
            genome.push_back((uint8_t)v);
        }
    }
    if (!next(f, &n_reads) || n_reads < 0) return 3;
    int lines = 0;
    for (int64_t r = 0; r < n_reads; ++r) {
        int64_t L = 0, n0 = 0, n1 = 0, nj = 0;
        if (!next(f, &L) || !next(f, &n0) || !next(f, &n1) || n0 < 0 || n0 > 64 || n1 < 0 || n1 > 64) return 3;
        const int n[2] = {(int)n0, (int)n1};
        std::vector<int64_t> rows[2], lrows[2];
        for (int m = 0; m < 2; ++m) {
            rows[m].assign((size_t)n[m] * kChRow + 1, 0);
            for (int i = 0; i < n[m] * kChRow; ++i) if (!next(f, &rows[m][(size_t)i])) return 3;
        }
        for (int m = 0; m < 2; ++m) {
            lrows[m].assign((size_t)n[m] * kLkRow + 1, 0);
            for (int i = 0; i < n[m] * kLkRow; ++i) if (!next(f, &lrows[m][(size_t)i])) return 3;
        }
        if (!next(f, &nj) || nj < 0 || nj > 64) return 3;
        std::vector<int64_t> jrows((size_t)nj * kJxRow + 1, 0);
        for (int64_t i = 0; i < nj * kJxRow; ++i) if (!next(f, &jrows[(size_t)i])) return 3;

        const int64_t* const lp[2] = {lrows[0].data(), lrows[1].data()};
        const int64_t* const rp[2] = {rows[0].data(), rows[1].data()};
        int64_t score = 0, row[kCcRow] = {0};
        uint64_t key = 0;
        if (!cc_best_path(lp, rp, n, min_path_score, &score, &key)) {
            printf("path %lld none\n", (long long)r); ++lines;
            row[0] = kCcNoPath;
        } else {
            const int minus = (int)(key >> 46) & 1, path = (int)(key & 63), nm = n[minus];
            uint64_t mask = 0;
            int chains = 0;
            for (int c = 0; c < nm; ++c) {
                const int64_t* lr = lp[minus] + (size_t)c * kLkRow;
                if (lr[4] != path) continue;
                ++chains;
                if (lr[3] == kLkBacksplice) mask |= (uint64_t)1 << lr[5];
            }
            const int links = __builtin_popcountll(mask);
            printf("path %lld %d %lld %d %d %d\n", (long long)r, minus, (long long)score, path, chains, links); ++lines;
            std::vector<int64_t> task((size_t)links * kJxTask + 1, 0);
            for (int c = 0; c < nm; ++c) {
                const int64_t* lr = lp[minus] + (size_t)c * kLkRow;
                if (lr[4] != path || lr[3] != kLkBacksplice) continue;
                if (lr[2] < 0 || lr[2] >= nm) { printf("circle_host: read %lld: a back-splice without a source\n", (long long)r); return 1; }
                cc_task(r, minus, rp[minus] + (size_t)lr[2] * kChRow, rp[minus] + (size_t)c * kChRow, (int)k, task.data() + (size_t)cc_ordinal(mask, (int)lr[5]) * kJxTask);
            }
            for (int t = 0; t < links; ++t) {
                const int64_t* tk = task.data() + (size_t)t * kJxTask;
                if (tk[2] < 0 || tk[2] >= n_contigs) { printf("circle_host: read %lld: contig out of range\n", (long long)r); return 1; }
                const int st = jx_status(tk[3], tk[4], tk[5], tk[6], max_span);
                printf("task %lld %lld %lld %lld %lld %lld %lld %lld %d %d %d\n", (long long)tk[0], (long long)tk[1], (long long)tk[2], (long long)tk[3], (long long)tk[4],
                       (long long)tk[5], (long long)tk[6], (long long)tk[7], cc_task_ok(tk, L, len[(size_t)tk[2]]) ? 1 : 0, st, st ? 0 : jx_class(tk[6] - tk[4]));
                ++lines;
            }
            if (links != nj) { printf("circle_host: read %lld: %d tasks, the checker made %lld rows\n", (long long)r, links, (long long)nj); return 1; }
            row[0] = links ? kCcFound : kCcNoBacksplice;
            row[9] = minus; row[10] = score; row[11] = chains; row[12] = links;
            if (links) {
                int refined = 0;
                const int w = cc_winner(jrows.data(), links, &refined);
                row[13] = refined;
                if (w < 0) row[0] = kCcNoJunction;
                else {
                    const int64_t* tk = task.data() + (size_t)w * kJxTask;
                    const int64_t* j = jrows.data() + (size_t)w * kJxRow;
                    int donor = 0, acceptor = 0;
                    cc_flanks(genome.data(), off[(size_t)tk[2]], len[(size_t)tk[2]], j[7], j[6], j[2] != 0, &donor, &acceptor);
                    row[1] = tk[2]; row[2] = j[7]; row[3] = j[6]; row[4] = j[2] != 0; row[5] = donor; row[6] = acceptor; row[7] = j[1];
                    row[8] = cc_read_pos(L, tk[4], j[3], minus); row[14] = w;
                }
            }
        }
        printf("row %lld", (long long)r);
        for (int i = 0; i < kCcRow; ++i) printf(" %lld", (long long)row[i]);
        printf("\n");
        ++lines;
    }
    fclose(f);
    // the order of two candidates on its own, field by field, and the codes of every dinucleotide and its reverse complement
    for (int64_t sa = -1; sa <= 1; ++sa)
        for (int ma = 0; ma < 2; ++ma)
            for (int64_t xa = 0; xa < 2; ++xa)
                for (int pa = 0; pa < 2; ++pa) {
                    const int64_t x = xa ? kLkLimit - 1 : 0;
                    printf("before %lld %d %lld %d %d\n", (long long)sa, ma, (long long)x, pa * 63, cc_path_before(sa, cc_tie_key(ma, x, pa * 63), 0, cc_tie_key(1, 0, 63)) ? 1 : 0);
                    ++lines;
                }
    for (int code = -1; code < 25; ++code) { printf("revcomp %d %d\n", code, cc_dinuc_revcomp(code)); ++lines; }
    printf("circle_host: %d lines: ok\n", lines);
    return 0;
}
