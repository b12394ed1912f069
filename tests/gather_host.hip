// gather_host.hip -- the gather of windows of the resident genome (gather_word, gather_combine, gather_move_word of
// csrc/genome_gather.h) on the CPU.  The kernel's lanes call gather_move_word and nothing else; this program, built with
// AddressSanitizer and UBSan (tests/test_gather_host.py), calls it for every destination word of every tile of a window, as the
// kernel's work items do, over a heap array of exactly the genome's allocation (its length rounded up the way the device allocator
// never rounds down: length + kGenomePad) and into a heap destination of exactly the padded window, so that the sanitizers report
// any load or store outside either.  It compares what arrives with a plain loop, one byte at a time: code = byte & 7, above 4 is 4,
// 3 - code where complemented and code < 4, letter t from base len - 1 - t where reversed.  Bytes behind the window's last letter
// must stay as they were.  Nothing here touches a GPU.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "genome_gather.h"

using namespace clh;

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;                   // the fixed seed
static uint32_t rnd()
{
    g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
    return (uint32_t)(g_rng >> 24);
}

static long g_windows = 0, g_words = 0;

// a genome byte as genome_encode_kernel may write it, and now and then one it never writes (codes 5..7, high bits)
static uint8_t genome_byte()
{
    const uint32_t r = rnd();
    if ((r & 63) == 0) return (uint8_t)(r >> 8);
    const uint32_t code = (r >> 8) % 5;
    if (code == 4) return (uint8_t)(4 | ((r >> 12) & 1 ? 16 : 0));
    return (uint8_t)(code | ((r >> 12) & 1 ? 8 : 0));
}

static int plain_code(int byte, int comp)
{
    int c = byte & 7;
    c = c > 4 ? 4 : c;
    return (comp && c < 4) ? 3 - c : c;
}

static void one_window(const uint8_t* codes, int64_t genome_len, int64_t off, int len, int flags)
{
    const int64_t cap = ((int64_t)len + kGatherWord - 1) & ~(int64_t)(kGatherWord - 1);
    // posix_memalign: the plan's buffer is 16-byte aligned, and ASan guards the bytes behind `cap`
    void* mem = nullptr;
    if (posix_memalign(&mem, kGatherWord, (size_t)(cap ? cap : kGatherWord))) { printf("gather_host: FAILED out of memory\n"); exit(1); }
    int8_t* dst = (int8_t*)mem;
    memset(dst, 0x55, (size_t)(cap ? cap : kGatherWord));
    const GatherTask t = {off, 0, len, flags, 0};
    const int64_t tiles = gather_tiles(len);
    for (int64_t tile = 0; tile < tiles; ++tile)
        for (int lane = 0; lane < 64; ++lane)
            for (int u = 0; u < kGatherTile / (64 * kGatherWord); ++u) {
                gather_move_word(codes, gather_src_cap(genome_len), t, tile * (kGatherTile / kGatherWord) + lane + 64 * u, dst, cap);
                ++g_words;
            }
    for (int64_t x = 0; x < cap; ++x) {
        int want = 0x55;
        if (x < len) want = plain_code(codes[off + ((flags & kGatherReverse) ? len - 1 - x : x)], flags & kGatherComplement);
        if (dst[x] != (int8_t)want) {
            printf("gather_host: FAILED window off %lld len %d flags %d: byte %lld is %d, want %d\n", (long long)off, len, flags, (long long)x, (int)dst[x], want);
            exit(1);
        }
    }
    free(mem);
    ++g_windows;
}

int main()
{
    static_assert(kGatherTile % (64 * kGatherWord) == 0, "a tile is whole words of a wave");
    const int lens_tile[] = {kGatherTile - 1, kGatherTile, kGatherTile + 1, 2 * kGatherTile - 1, 2 * kGatherTile, 2 * kGatherTile + 1};
    // genomes whose length is every residue mod 16, so that windows ending at the last byte meet every alignment of the pad
    for (int extra = 0; extra < 16; ++extra) {
        const int64_t genome_len = 3 * kGatherTile + 100 + extra;
        uint8_t* codes = nullptr;
        if (posix_memalign((void**)&codes, kGatherWord, (size_t)(genome_len + kGenomePad))) return 1;      // the genome's base is aligned
        for (int64_t x = 0; x < genome_len + kGenomePad; ++x) codes[x] = x < genome_len ? genome_byte() : (uint8_t)0xff;
        for (int flags = 0; flags < 4; ++flags) {
            for (int len = 0; len <= 70; ++len) {
                for (int off = 0; off < 48; ++off) one_window(codes, genome_len, off, len, flags);            // every off mod 16, byte 0 included
                one_window(codes, genome_len, genome_len - len, len, flags);                                     // ending at the last byte
            }
            for (int len : lens_tile) {
                for (int off = 0; off < 16; ++off) one_window(codes, genome_len, off, len, flags);
                one_window(codes, genome_len, genome_len - len, len, flags);
            }
            one_window(codes, genome_len, 0, (int)genome_len, flags);                                            // the whole genome
        }
        free(codes);
    }
    // decode: every byte value in every position of a word
    for (uint32_t b = 0; b < 256; ++b)
        for (int pos = 0; pos < 4; ++pos)
            for (int comp = 0; comp < 2; ++comp) {
                const uint32_t w = (b << (8 * pos)) | (0x04030201u & ~(0xffu << (8 * pos)));
                const uint32_t got = gather_decode4(w, comp ? 0xffffffffu : 0u);
                for (int k = 0; k < 4; ++k)
                    if ((int)((got >> (8 * k)) & 0xff) != plain_code((int)((w >> (8 * k)) & 0xff), comp)) {
                        printf("gather_host: FAILED decode of %08x comp %d: %08x\n", w, comp, got);
                        return 1;
                    }
            }
    printf("gather_host: tile %d, %ld windows, %ld words: ok\n", kGatherTile, g_windows, g_words);
    return 0;
}
