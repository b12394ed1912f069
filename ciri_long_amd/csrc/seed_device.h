// seed_device.h -- K7: what the host side, the sketch, look-up and chain kernels (seed.hip), the link, junction and circle kernels
// (seed_link.hip, seed_junction.hip, seed_circle.hip), the sort plumbing (seed_sort.hip) and the stand-alone host programs
// tests/seed_host.hip, link_host.hip, junction_host.hip and circle_host.hip share.  The definitions are those of DESIGN.md section 4 (K7): they are independent of
// the order in which positions are visited, so that the kernels and the plain checker tests/seed_check.py agree bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace clh {

static constexpr int kSdKMin = 4, kSdKMax = 28, kSdWMin = 1, kSdWMax = 64;
static constexpr int kSdRound = 64;                     // positions a wave decides at once: lane l takes position round * 64 + l
static constexpr int kSdItem = 16 * kSdRound;           // positions of one work item (one wave)
static constexpr int kSdItemsPerBlock = 4;              // work items of one workgroup (256 threads)
static constexpr int kSdKeysCap = kSdItem + 2 * (kSdWMax - 1);      // keys an item holds in LDS: its positions and w' - 1 on either side
static constexpr int kSdLettersCap = kSdKeysCap + kSdKMax - 1;      // letters under those keys
static constexpr uint64_t kSdNoKey = ~(uint64_t)0;      // a position without a valid k-mer; as (key << 1 | strand) it is above every valid one
static constexpr int kSdYBits = 24;                     // an anchor's sort word is x << 24 | y: reads of 2^24 letters and more are refused
static constexpr int kChLookbackMax = 64, kChMaxChains = 64;
static constexpr int64_t kChUnwritten = (int64_t)0x8080808080808080ull;    // what the chain rows are filled with before a run
static constexpr int kChRow = 10, kChSeg = 4;           // int64 per chain row / per segment header

// the 64-bit integer mix with every step masked to 2k bits: a bijection on [0, 2^2k)
__host__ __device__ inline uint64_t sd_mix(uint64_t h, uint64_t m)
{
    h = (~h + (h << 21)) & m;
    h ^= h >> 24;
    h = (h + (h << 3) + (h << 8)) & m;
    h ^= h >> 14;
    h = (h + (h << 2) + (h << 4)) & m;
    h ^= h >> 28;
    h = (h + (h << 31)) & m;
    return h;
}

// The rolling state of one stretch of letters: f the forward packing of the last k letters (first base most significant), r that of
// their reverse complement, run the letters since the last code >= 4.
struct SdRoll { uint64_t f, r; int run; };
__host__ __device__ inline void sd_roll_init(SdRoll* s) { s->f = s->r = 0; s->run = 0; }
// code: bits 0-2 of a resident genome byte or a read code; anything above 3 is no base
__host__ __device__ inline void sd_roll_push(SdRoll* s, int code, int k, uint64_t m)
{
    const int c = code & 7;
    if (c > 3) { s->run = 0; s->f = s->r = 0; return; }
    s->f = ((s->f << 2) | (uint64_t)c) & m;
    s->r = (s->r >> 2) | ((uint64_t)(3 - c) << (2 * (k - 1)));
    s->run = s->run < k ? s->run + 1 : k;
}
// after the letter at position p + k - 1 was pushed: (key << 1 | strand) of position p, kSdNoKey where there is no valid k-mer
__host__ __device__ inline uint64_t sd_roll_key(const SdRoll& s, int k, uint64_t m)
{
    if (s.run < k || s.f == s.r) return kSdNoKey;
    return (sd_mix(s.f < s.r ? s.f : s.r, m) << 1) | (uint64_t)(s.f > s.r);
}

// The selection rule for one position: v[i] = (key << 1 | strand) or kSdNoKey for the positions [lo, hi) of the sequence that the caller
// holds, v[0] being position lo; p in [lo, hi); wp = min(w, P).  The caller holds at least the wp - 1 positions on either side of p that
// exist.  a and b are the runs left and right of p whose key is invalid or >= key[p], each at most wp - 1.
__host__ __device__ inline bool sd_selected(const uint64_t* v, int64_t lo, int64_t hi, int64_t p, int wp)
{
    const uint64_t me = v[p - lo];
    if (me == kSdNoKey) return false;
    const uint64_t key = me >> 1;
    int a = 0, b = 0;
    while (a < wp - 1 && p - a - 1 >= lo && (v[p - a - 1 - lo] >> 1) >= key) ++a;
    while (a + b < wp - 1 && p + b + 1 < hi && (v[p + b + 1 - lo] >> 1) >= key) ++b;
    return a + b + 1 >= wp;
}

// chain transition: what anchor j adds to anchor i at distances dx, dy (both > 0): min(dx, dy, k) - beta(|dx - dy|)
__host__ __device__ inline int64_t ch_beta(int64_t d, int k)
{
    if (d <= 0) return 0;
    const int lg = 63 - __builtin_clzll((unsigned long long)d);      // floor(log2 d)
    return ((int64_t)k * d + 99) / 100 + lg / 2;
}
__host__ __device__ inline int64_t ch_gain(int64_t dx, int64_t dy, int k)
{
    int64_t g = dx < dy ? dx : dy;
    if (g > k) g = k;
    return g - ch_beta(dx > dy ? dx - dy : dy - dx, k);
}

// ---- links between the chains of one segment (seed_link.hip; tests/link_check.py) --------------------------
static constexpr int kLkRow = 8, kLkSeg = 4;            // int64 per link row / per link header
static constexpr int64_t kLkNone = INT64_MIN;           // no link
static constexpr int64_t kLkLimit = (int64_t)1 << 40;   // coordinates, scores and the two costs lie in [0, 2^40): no sum below can overflow
enum { kLkColinear = 1, kLkIntron = 2, kLkBacksplice = 3 };
struct LkChain { int64_t g, score, x0, x1, y0, y1; };
struct LkParams { int64_t max_query_gap, max_overlap, max_skew, max_intron, max_circle, intron_cost, backsplice_cost; };

// the order of the chains of a segment: (y0, y1, x0, c) ascending, c the chain's index
__host__ __device__ inline bool lk_before(const LkChain& a, int ca, const LkChain& b, int cb)
{
    if (a.y0 != b.y0) return a.y0 < b.y0;
    if (a.y1 != b.y1) return a.y1 < b.y1;
    if (a.x0 != b.x0) return a.x0 < b.x0;
    return ca < cb;
}

// The link j -> i (j before i in the order above, which the caller sees to): what it adds to F_j, that is -(cost + read overlap), always
// <= 0, with its kind in *kind; kLkNone and kind 0 where the link is not admissible.
__host__ __device__ inline int64_t lk_link(const LkChain& j, const LkChain& i, const LkParams& p, int k, int* kind)
{
    *kind = 0;
    if (j.g != i.g || i.y0 <= j.y0 || i.y1 <= j.y1) return kLkNone;
    const int64_t q = i.y0 - j.y1;
    if (q > p.max_query_gap || -q > p.max_overlap) return kLkNone;
    const int64_t d = (i.x0 - j.x1) - q, ad = d < 0 ? -d : d;
    int64_t cost;
    if (ad <= p.max_skew) { *kind = kLkColinear; cost = ch_beta(ad, k); }
    else if (d > 0 && d <= p.max_intron) { *kind = kLkIntron; cost = p.intron_cost; }
    else if (d < 0 && j.x1 - i.x0 > 0 && j.x1 - i.x0 <= p.max_circle) { *kind = kLkBacksplice; cost = p.backsplice_cost; }
    else return kLkNone;
    return -(cost + (q < 0 ? -q : 0));
}

// ---- a back-splice junction refined to the base (seed_junction.hip; tests/junction_check.py) ---------------
static constexpr int kJxTask = 8, kJxRow = 12;          // int64 per task (read, minus, contig, xd, yd, xa, ya, strand) / per result row
static constexpr int kJxMaxSpan = 512, kJxMaxSlack = 64;
static constexpr int kJxWaves = 4;                      // tasks of one workgroup: the waves share nothing
static constexpr int kJxClasses = 4;                    // class c takes m <= kJxClassBase << c with 1 << c rows per lane
static constexpr int kJxClassBase = 64;                  // the rows of class 0: one per lane
static_assert((kJxClassBase << (kJxClasses - 1)) == kJxMaxSpan, "the last class takes max_span");
static constexpr int kJxSiteOther = 64, kJxSites = 65;  // the site table of clh_device.h (kSpOther, kSpSites): start+, end+, start-, end-, other
// (2 max_span + slack) max(match, mismatch, gap_open, gap_extend) + intron_open + dmax + amax stays below this: a side score less a
// site cost then lies inside (-2^20, 2^20) and stands, times 1024, above a 10-bit column index in one 32-bit key
static constexpr int64_t kJxBound = (int64_t)1 << 20;
static constexpr int kJxIndexBits = 10, kJxIndexMask = (1 << kJxIndexBits) - 1;      // columns 0 .. 512 + 64

__host__ __device__ inline int64_t jx_class_bound(int c) { return (int64_t)kJxClassBase << c; }
__host__ __device__ inline int jx_class(int64_t m)
{
    int c = 0;
    while (c < kJxClasses - 1 && m > jx_class_bound(c)) ++c;
    return c;
}
// 0: refined; 1: m = ya - yd above max_span; 2: no read letter between the anchors, or the acceptor anchor not below the donor anchor
__host__ __device__ inline int jx_status(int64_t xd, int64_t yd, int64_t xa, int64_t ya, int64_t max_span)
{
    if (ya - yd > max_span) return 1;
    if (ya - yd < 1 || xa >= xd) return 2;
    return 0;
}
// the letters of D = contig[xd : min(xd + m + slack, len)) and of A = contig[max(0, xa - m - slack) : xa); 0 <= xd, xa <= len
__host__ __device__ inline int64_t jx_nd(int64_t xd, int64_t m, int64_t slack, int64_t len)
{
    const int64_t e = xd + m + slack < len ? xd + m + slack : len;
    return e > xd ? e - xd : 0;
}
__host__ __device__ inline int64_t jx_na(int64_t xa, int64_t m, int64_t slack)
{
    const int64_t s = xa - m - slack > 0 ? xa - m - slack : 0;
    return xa > s ? xa - s : 0;
}
// letter x of the contig that lies at [off, off + len) of the genome, as genome_gather.h reads it: bits 0-2, clamped to 4; 4 outside
__host__ __device__ inline int jx_letter(const uint8_t* genome, int64_t off, int64_t len, int64_t x)
{
    if (x < 0 || x >= len) return 4;
    const int c = genome[off + x] & 7;
    return c > 4 ? 4 : c;
}
// the cost of the dinucleotide at contig positions (p, p + 1) as a run's start (part 0, p = a) or end (part 1, p = b - 1) on strand
// + (minus 0) or - (minus 1); `other` where it holds a code >= 4 or leaves the contig
__host__ __device__ inline int jx_site(const int32_t* site, const uint8_t* genome, int64_t off, int64_t len, int64_t p, int part, int minus)
{
    const int a = jx_letter(genome, off, len, p), b = jx_letter(genome, off, len, p + 1);
    if (a > 3 || b > 3) return site[kJxSiteOther];
    return site[32 * minus + 16 * part + 4 * a + b];
}
// letter y of S, the read of L letters as the strand reads it
__host__ __device__ inline int jx_read_letter(const int8_t* read, int64_t L, int64_t y, int minus)
{
    if (y < 0 || y >= L) return 4;
    const int c = minus ? read[L - 1 - y] : read[y];
    return minus && c < 4 ? 3 - c : c;
}

// All device pointers.  Tasks order[first[c] .. first[c + 1]) are those of class c; out[n][kJxRow] is marker-filled by the caller.
struct JxLaunch {
    const uint8_t* genome; const int64_t* ctg_off; const int64_t* ctg_len;
    const int8_t* reads; const int64_t* read_off;
    const int64_t* task; const int64_t* order; int64_t first[kJxClasses + 1];
    const int32_t* site;                                // kJxSites costs
    int32_t match, mismatch, go, ge, io, slack, max_span;
    int64_t* out;
};
hipError_t launch_seed_junction(const JxLaunch& l, hipStream_t stream);
// the letters (jx_letter's codes) of n short spans of the genome: span i is len[i] bytes from off[i] and goes to out + at[i]; one lane a span
hipError_t launch_genome_letters(const uint8_t* genome, int64_t genome_len, const int64_t* off, const int64_t* len, const int64_t* at, int64_t n, int8_t* out,
                                 hipStream_t stream);

// ---- the circles of a read batch (seed_circle.hip; tests/circle_check.py) ---------------------------------
static constexpr int kCcRow = 16, kCcTable = 10;        // int64 per circle row (one per read) / per table row (one per distinct circle)
static constexpr int kCcSel = 8;                        // int64 per read between select and finalise: state, minus, score, chains, links, 0, 0, 0
static constexpr int kCcWaves = 4;                      // reads of one workgroup of the select kernel: the waves share nothing
static constexpr int kCcContigBits = 23;                // the table's sort word is (another status) << 63 | contig << 40 | start
enum { kCcFound = 0, kCcNoPath = 1, kCcNoBacksplice = 2, kCcNoJunction = 3, kCcBad = 4 };      // kCcBad never leaves the device: the row stays unwritten
static constexpr int64_t kCcNoScore = INT64_MIN;        // a lane without a candidate path

// The best path of a read is the least under (-score, minus, x_first of its pos-0 chain, path index); the last three make one word.
__host__ __device__ inline uint64_t cc_tie_key(int minus, int64_t x_first, int path)
{
    return ((uint64_t)(minus != 0) << 46) | ((uint64_t)x_first << 6) | (uint64_t)path;       // x_first in [0, 2^40), path in [0, 64)
}
__host__ __device__ inline bool cc_path_before(int64_t score_a, uint64_t key_a, int64_t score_b, uint64_t key_b)
{
    return score_a != score_b ? score_a > score_b : key_a < key_b;
}
// The best of the candidate paths of one read, stated serially over its two segments one after the other (the statement that
// tests/circle_host.hip runs; seed_circle_select_kernel reduces the same (score, key) pairs per lane and across the wave): lrows_m / rows_m are the link and the
// chain rows of segment m (n_m of them); a candidate is a chain with pos == 0 whose path scores at least min_path_score.
// -> true and (score, key) of the best, or false
__host__ __device__ inline bool cc_best_path(const int64_t* const lrows[2], const int64_t* const rows[2], const int n[2], int64_t min_path_score, int64_t* score,
                                             uint64_t* key)
{
    bool any = false;
    for (int m = 0; m < 2; ++m)
        for (int c = 0; c < n[m]; ++c) {
            const int64_t* lr = lrows[m] + (int64_t)c * kLkRow;
            if (lr[5] != 0 || lr[6] < min_path_score) continue;
            const uint64_t kc = cc_tie_key(m, rows[m][(int64_t)c * kChRow + 5], (int)lr[4]);
            if (!any || cc_path_before(lr[6], kc, *score, *key)) { *score = lr[6]; *key = kc; any = true; }
        }
    return any;
}
// the K7j task of the back-splice link j -> i of read `read` on strand `minus`: row_j, row_i are the two chain rows (kChRow)
__host__ __device__ inline void cc_task(int64_t read, int minus, const int64_t* row_j, const int64_t* row_i, int k, int64_t* task)
{
    task[0] = read; task[1] = minus; task[2] = row_i[2];
    task[3] = row_j[7] - k; task[4] = row_j[8] - k;     // the donor anchor: the start of the source chain's last k-mer
    task[5] = row_i[5] + k; task[6] = row_i[6] + k;     // the acceptor anchor: the end of the target chain's first k-mer
    task[7] = 0;
}
// what clh_seed_junction_batch admits of a task: L the read's letters, len the contig's
__host__ __device__ inline bool cc_task_ok(const int64_t* task, int64_t L, int64_t len)
{
    return task[4] >= 0 && task[4] <= L && task[6] >= 0 && task[6] <= L && task[3] >= 0 && task[3] <= len && task[5] >= 0 && task[5] <= len;
}
// the ordinal of the link into the chain at `pos` among the path's back-splice links: mask has bit p set for every such chain at pos p
__host__ __device__ inline int cc_ordinal(uint64_t mask, int pos) { return __builtin_popcountll(mask & (((uint64_t)1 << pos) - 1)); }
// the winner among the cnt K7j rows of a path, in path order: the greatest J of status 0, the first among equals; -1 where none is refined
__host__ __device__ inline int cc_winner(const int64_t* jrows, int cnt, int* refined)
{
    int best = -1;
    *refined = 0;
    for (int t = 0; t < cnt; ++t) {
        const int64_t* r = jrows + (int64_t)t * kJxRow;
        if (r[0] != 0) continue;
        ++*refined;
        if (best < 0 || r[1] > jrows[(int64_t)best * kJxRow + 1]) best = t;
    }
    return best;
}
// the dinucleotide at contig positions (p, p + 1) as 5 c0 + c1 (jx_letter's codes); -1 where fewer than two of its letters lie inside the contig
__host__ __device__ inline int cc_dinuc(const uint8_t* genome, int64_t off, int64_t len, int64_t p)
{
    if (p < 0 || p + 2 > len) return -1;
    return 5 * jx_letter(genome, off, len, p) + jx_letter(genome, off, len, p + 1);
}
__host__ __device__ inline int cc_dinuc_revcomp(int code)
{
    if (code < 0) return -1;
    const int c0 = code / 5, c1 = code % 5;
    return 5 * (c1 < 4 ? 3 - c1 : 4) + (c0 < 4 ? 3 - c0 : 4);
}
// donor and acceptor codes of the circle [start, end) on transcript strand `sminus`, as the transcript reads them
__host__ __device__ inline void cc_flanks(const uint8_t* genome, int64_t off, int64_t len, int64_t start, int64_t end, int sminus, int* donor, int* acceptor)
{
    const int after = cc_dinuc(genome, off, len, end), before = cc_dinuc(genome, off, len, start - 2);
    *donor = sminus ? cc_dinuc_revcomp(before) : after;
    *acceptor = sminus ? cc_dinuc_revcomp(after) : before;
}
// the split in the read as given: y = yd + t in the read as the strand reads it
__host__ __device__ inline int64_t cc_read_pos(int64_t L, int64_t yd, int64_t t, int minus) { return minus ? L - (yd + t) : yd + t; }

// All device pointers.  The share holds reads [read0, read0 + nreads): seg, rows, lseg, lrows are the chain and link rows of its 2 nreads
// segments; read r of the share owns the task slots [r slots, (r + 1) slots), slots = max(max_chains - 1, 1), of which the first
// sel[r][4] are filled in path order.  cls[slot] is the K7j class of a filled slot and -1 of an empty one; count[c] (zeroed by the caller)
// receives the tasks of class c; order and first[] of the JxLaunch are made of them by launch_seed_circle_route.
struct CcLaunch {
    const int64_t* seg; const int64_t* rows; const int64_t* lseg; const int64_t* lrows;
    int32_t nreads, read0, max_chains, slots, k, n_contigs, max_span;
    int64_t min_path_score;
    const int64_t* read_off;                            // [reads of the batch + 1]
    const uint8_t* genome; const int64_t* ctg_off; const int64_t* ctg_len;
    int64_t* sel; int64_t* task; int32_t* cls;
    unsigned long long* count;                          // [2 kJxClasses]: the tasks of each class, then the route kernel's cursors
    int64_t* order;                                     // [nreads slots]
    const int64_t* junction;                            // [nreads slots][kJxRow]: what K7j left
    int64_t* circle;                                    // [reads of the batch][kCcRow], marker-filled by the caller
};
hipError_t launch_seed_circle_select(const CcLaunch& l, hipStream_t stream);
hipError_t launch_seed_circle_route(const CcLaunch& l, hipStream_t stream);
hipError_t launch_seed_circle_finalise(const CcLaunch& l, hipStream_t stream);
// The table of n circle rows: sort words, the gather between the two sort passes, head flags, and the scatter.  perm is the reads in
// ascending (contig, start, end, strand) with the rows of another status last; head[n + 1] and first[n + 1] its flags and their exclusive scan.
hipError_t launch_seed_circle_keys(const int64_t* circle, int64_t n, uint64_t* key_lo, uint64_t* key_hi, uint64_t* read, hipStream_t stream);
hipError_t launch_seed_circle_gather(const uint64_t* key_hi, const uint64_t* perm, int64_t n, uint64_t* out, hipStream_t stream);
hipError_t launch_seed_circle_heads(const int64_t* circle, const uint64_t* perm, int64_t n, int32_t* head, hipStream_t stream);
hipError_t launch_seed_circle_table(const int64_t* circle, const uint64_t* perm, const int32_t* head, const int64_t* first, int64_t n, int64_t* table,
                                    int64_t* circle_of_read, hipStream_t stream);

// ---- launches (seed.hip) ------------------------------------------------------------------------------------------------------
// The sequences of one sketch: sequence s is the len[s] bytes from off[s] of `codes`; its positions [0, len - k] are cut into work items of
// kSdItem positions; item_seq[i] names the sequence of item i and seq_item0[s] its first item (seq_item0[nseq] = items).  All device pointers.
struct SdSketch {
    const uint8_t* codes; int64_t codes_len;
    const int64_t* off; const int64_t* len; int32_t nseq;
    const int32_t* item_seq; const int64_t* seq_item0; int64_t nitems;
    int32_t k, w;
    int32_t global_pos;                                 // 1: a position is written genome-wide (off[s] + p), 0: inside its sequence
};
// count: item_count[i] = minimizers of item i.  fill: with item_off the exclusive scan of the counts, entry e gets keys[e] = key, vals[e] =
// position << 1 | strand, and, where seq_of is given, seq_of[e] = the sequence; entries are in (sequence, position) order; cap = entries
hipError_t launch_seed_sketch_count(const SdSketch& s, int32_t* item_count, hipStream_t stream);
hipError_t launch_seed_sketch_fill(const SdSketch& s, const int64_t* item_off, uint64_t* keys, uint64_t* vals, int32_t* seq_of, int64_t cap, hipStream_t stream);
// sorted keys of n entries: stats[0] += distinct keys, stats[1] += keys with more than max_occ entries (stats zeroed by the caller)
hipError_t launch_seed_index_stats(const uint64_t* keys, int64_t n, int32_t max_occ, unsigned long long* stats, hipStream_t stream);
// per minimizer e of the reads: lo[e] = first entry of the index with its key, cnt[e] = anchors it gives (0 where there are more than max_occ),
// rep[e] = 1 where there are more than max_occ
hipError_t launch_seed_lookup(const uint64_t* idx_keys, int64_t n_idx, int32_t max_occ, const uint64_t* rkeys, int64_t nmin, int64_t* lo, int32_t* cnt,
                              uint8_t* rep, hipStream_t stream);
// per read r (n + 1 of them, the last for the totals): read_aoff[r] = aoff[item_off[seq_item0[r]]], and for r < n repetitive[r] = the sum of rep over its minimizers
hipError_t launch_seed_per_read(const int64_t* seq_item0, const int64_t* item_off, const int64_t* aoff, const uint8_t* rep, int32_t n, int64_t* read_moff,
                                int64_t* read_aoff, int32_t* repetitive, hipStream_t stream);
// anchors of the minimizers [m0, m1): anchor aoff[e] - a0 + t (t-th entry of the index from lo[e]) gets k1 = read << 1 | minus, k2 = x << kSdYBits | y; cap = anchors of the share
hipError_t launch_seed_anchor_fill(const uint64_t* idx_vals, int64_t n_idx, const uint64_t* rvals, const int32_t* seq_of, const int64_t* read_len, const int64_t* lo,
                                   const int32_t* cnt, const int64_t* aoff, int64_t m0, int64_t m1, int64_t a0, int32_t k, uint64_t* k1, uint64_t* k2, int64_t cap,
                                   hipStream_t stream);

struct ChParams {
    const uint64_t* k1; const uint64_t* k2; int64_t n_anchors;       // the share's anchors in (read, minus, x, y) order
    int32_t read0, nseg;                                             // segment s of the share is (read0 + s / 2, s & 1)
    const int64_t* ctg_off; const int64_t* ctg_len; int32_t n_contigs;
    int32_t k, lookback, max_chains, max_attempts, min_score, min_anchors;
    int64_t max_gap, max_skew;
    int64_t* seg_bounds;                                             // [nseg + 1], made by launch_seed_segments
    int32_t* f; int32_t* p; uint8_t* used;                           // [n_anchors] each
    int64_t* seg; int64_t* rows;                                     // [nseg][kChSeg], [nseg][max_chains][kChRow], marker-filled by the caller
};
hipError_t launch_seed_segments(const ChParams& c, hipStream_t stream);
hipError_t launch_seed_chain(const ChParams& c, hipStream_t stream);

// Links (seed_link.hip): segment s has its chains in seg[s][0] (chain header) and rows[s][0 .. max_chains) (chain rows); lseg[nseg][kLkSeg]
// and lrows[nseg][max_chains][kLkRow] are marker-filled by the caller.  All device pointers; max_chains in 1..64.
struct LkLaunch {
    const int64_t* seg; const int64_t* rows; int32_t nseg, max_chains, k;
    LkParams p;
    int64_t* lseg; int64_t* lrows;
};
hipError_t launch_seed_link(const LkLaunch& l, hipStream_t stream);

// ---- plumbing (seed_sort.hip): rocPRIM's device radix sort and scan -------------------------------------------------------------
size_t seed_sort_temp_bytes(int64_t n);
// stable sort of (keys, vals) on key bits [0, bits): the result is in keys_out / vals_out
hipError_t seed_sort_pairs(void* temp, size_t temp_bytes, const uint64_t* keys_in, uint64_t* keys_out, const uint64_t* vals_in, uint64_t* vals_out, int64_t n, int bits,
                           hipStream_t stream);
size_t seed_scan_temp_bytes(int64_t n);
hipError_t seed_scan_counts(void* temp, size_t temp_bytes, const int32_t* counts, int64_t* out, int64_t n, hipStream_t stream);     // exclusive, 64-bit sums

}  // namespace clh
