// genome_gather.h -- K5's gather: windows of the resident genome copied into a pair plan's reference buffer as plain codes 0..4,
// read forwards or backwards, complemented or not.  Everything here but the launcher is __host__ __device__: genome.hip's kernel
// and tests/gather_host.hip (a CPU program under AddressSanitizer and UBSan) run the same text.
//
// A task is one window.  Its destination starts on a 16-byte boundary (the plan pads), so the window is a row of 16-byte destination
// words; word j holds the letters t = 16 j .. 16 j + 15 of the window as the pair kernels will read them.  Forwards, letter t is
// source byte src_off + t; backwards (flag 1) it is source byte src_off + len - 1 - t.  Either way the 16 source bytes of a
// destination word are consecutive, [s, s + 16), and lie in at most two aligned 16-byte words of the genome: the word at s & ~15 and
// the next.  gather_word says which, how far to shift across them, how many of the 16 bytes are letters of the window (the tail),
// and where they go; gather_combine shifts, reverses by swapping whole 32-bit words and their bytes, and decodes four codes per
// 32-bit operation.  A source word that lies outside the genome's allocation is not loaded: its bytes are zeros, and every one of
// them falls on a tail position that is not stored.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CLH_HD __host__ __device__
#else
#define CLH_HD
#endif

namespace clh {

static constexpr int kGatherReverse = 1, kGatherComplement = 2;      // GatherTask::flags
static constexpr int kGatherWord = 16;                               // bytes a lane loads and stores at once
static constexpr int kGatherTile = 2048;                             // destination bytes of one work item (one wave: 2 words per lane)
static constexpr int kGenomePad = 64;                                // bytes the genome's allocation holds behind its last base

struct GatherTask {
    int64_t src_off;        // first base of the window in the genome
    int64_t dst_off;        // first byte of the window in the destination, a multiple of 16
    int32_t len;
    int32_t flags;          // bit 0: reversed, bit 1: complemented
    int64_t first_tile;     // the index of the task's first work item: the tiles of all tasks are numbered in task order
};

CLH_HD inline int64_t gather_tiles(int64_t len) { return (len + kGatherTile - 1) / kGatherTile; }
// the bytes of the genome's allocation that whole aligned words may be loaded from
CLH_HD inline int64_t gather_src_cap(int64_t genome_len) { return (genome_len + kGenomePad) & ~(int64_t)(kGatherWord - 1); }

struct GatherWord {
    int64_t src[2];         // the two aligned source words (byte offsets into the genome); -1: not loaded, its bytes are zeros
    int shift;              // the destination word is bytes [shift, shift + 16) of the two words side by side
    int nvalid;             // letters of the window in this word, 0..16; fewer than 16: the tail, stored byte by byte
    int64_t dst;            // where the word goes
};

// destination word j of task t; src_cap: gather_src_cap of the genome
CLH_HD inline GatherWord gather_word(const GatherTask& t, int64_t j, int64_t src_cap)
{
    GatherWord g;
    const int64_t left = (int64_t)t.len - kGatherWord * j;
    g.nvalid = left <= 0 || j < 0 ? 0 : (left < kGatherWord ? (int)left : kGatherWord);
    g.dst = t.dst_off + kGatherWord * j;
    // backwards, the word's last source byte is src_off + len - 1 - 16 j and its first lies 15 in front of it: in a tail that is
    // before the window, and may be before the genome
    const int64_t s = (t.flags & kGatherReverse) ? t.src_off + left - kGatherWord : t.src_off + kGatherWord * j;
    const int64_t a = s & ~(int64_t)(kGatherWord - 1);               // rounds down, below zero too
    g.shift = (int)(s - a);
    g.src[0] = (a >= 0 && a + kGatherWord <= src_cap) ? a : -1;
    g.src[1] = (g.shift != 0 && a + kGatherWord >= 0 && a + 2 * kGatherWord <= src_cap) ? a + kGatherWord : -1;
    if (g.nvalid == 0) g.src[0] = g.src[1] = -1;
    return g;
}

// four genome bytes -> four codes 0..4: bits 0-2 of each, 5..7 clamped to 4; the case and N bits are dropped.  comp: all ones to
// complement (3 - c where c < 4), zero to leave
CLH_HD inline uint32_t gather_decode4(uint32_t w, uint32_t comp)
{
    uint32_t x = w & 0x07070707u;
    const uint32_t above = (x >> 2) & ((x >> 1) | x) & 0x01010101u;      // bit 2 and one of bits 0, 1: a code above 4
    x &= ~(above * 3u);
    const uint32_t base = (~x >> 2) & 0x01010101u;                       // bit 2 clear: a base, whose complement is code ^ 3
    return x ^ ((base * 3u) & comp);
}

// lo, hi: the two source words as four little-endian 32-bit words each -> out: the destination word
CLH_HD inline void gather_combine(const uint32_t lo[4], const uint32_t hi[4], int shift, int flags, uint32_t out[4])
{
    const int sw = shift >> 2, sb = 8 * (shift & 3);
    uint32_t f[7];                                                       // the eight words shifted by the odd bytes
    for (int i = 0; i < 7; ++i) {
        const uint32_t a = i < 4 ? lo[i] : hi[i - 4], b = i + 1 < 4 ? lo[i + 1] : hi[i - 3];
        f[i] = (uint32_t)((((uint64_t)b << 32) | a) >> sb);
    }
    uint32_t v[4];
    for (int i = 0; i < 4; ++i) v[i] = sw == 0 ? f[i] : (sw == 1 ? f[i + 1] : (sw == 2 ? f[i + 2] : f[i + 3]));
    const uint32_t comp = (flags & kGatherComplement) ? 0xffffffffu : 0u;
    const bool rev = (flags & kGatherReverse) != 0;
    for (int i = 0; i < 4; ++i) {
        const uint32_t w = rev ? __builtin_bswap32(v[3 - i]) : v[i];     // byte 15 - b of the word becomes byte b
        out[i] = gather_decode4(w, comp);
    }
}

// destination word j of task t, from the genome's codes to dst: what one lane of the kernel does.  Loads are whole aligned words
// inside src_cap, stores lie inside dst_cap: a whole aligned word, or the tail byte by byte.
CLH_HD inline void gather_move_word(const uint8_t* codes, int64_t src_cap, const GatherTask& t, int64_t j, int8_t* dst, int64_t dst_cap)
{
    const GatherWord g = gather_word(t, j, src_cap);
    if (g.nvalid == 0 || g.dst < 0) return;
    uint32_t lo[4] = {0, 0, 0, 0}, hi[4] = {0, 0, 0, 0}, o[4];
    if (g.src[0] >= 0) __builtin_memcpy(lo, __builtin_assume_aligned(codes + g.src[0], kGatherWord), kGatherWord);
    if (g.src[1] >= 0) __builtin_memcpy(hi, __builtin_assume_aligned(codes + g.src[1], kGatherWord), kGatherWord);
    gather_combine(lo, hi, g.shift, t.flags, o);
    if (g.nvalid == kGatherWord && (g.dst & (kGatherWord - 1)) == 0 && g.dst + kGatherWord <= dst_cap)
        __builtin_memcpy(__builtin_assume_aligned(dst + g.dst, kGatherWord), o, kGatherWord);
    else
        for (int c = 0; c < kGatherWord; ++c)
            if (c < g.nvalid && g.dst + c < dst_cap) dst[g.dst + c] = (int8_t)(o[c >> 2] >> (8 * (c & 3)));
}

}  // namespace clh
