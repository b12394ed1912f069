// clh_api.hip -- host side of libclh.so: contexts, batch plans, launches, and the reference's legacy symbols.
// Public interface and the reference lines each entry point replaces: include/ciri_long_hip.h, include/ssw_legacy.h.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/ciri_long_hip.h"
#include "../../include/ssw_legacy.h"
#include "clh_device.h"
#include "ssw_pairs.h"

static thread_local std::string g_err;
static thread_local int g_code = CLH_E_ARG;            // the code of the last failure: what a batch call returns when its plan was refused
static int fail(int code, const std::string& m) { g_err = m; g_code = code; return code; }
#define HIPCHK(expr)                                                                         \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess) return fail(CLH_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

extern "C" const char* clh_last_error(void) { return g_err.c_str(); }
extern "C" const char* clh_version(void) { return "libclh 0.1 (gfx950)"; }

extern "C" int clh_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// ------------------------------------------------------------------------------------------------------------
// context: device + stream + a small caching allocator (hipMalloc is milliseconds; the legacy path calls us per alignment)
// ------------------------------------------------------------------------------------------------------------
struct clh_ctx {
    int device;
    int n_cu = 256;                                      // compute units (persistent launches are sized by it)
    hipStream_t stream;
    hipStream_t side[3] = {nullptr, nullptr, nullptr};   // the read-length classes of a batch are launched on 4 streams so their tails overlap
    hipEvent_t fork_ev = nullptr, join_ev[3] = {nullptr, nullptr, nullptr};
    std::mutex mu;
    std::vector<std::pair<size_t, void*>> cache;
    int64_t last_poa_stats[16] = {0};                  // clh_ccs_plan_stats of the last clh_poa_batch (its plan lives only inside the call)

    void* alloc(size_t bytes)
    {
        if (bytes == 0) bytes = 256;
        std::lock_guard<std::mutex> g(mu);
        int best = -1;
        for (size_t i = 0; i < cache.size(); ++i)
            if (cache[i].first >= bytes && cache[i].first <= bytes * 4 + 4096 && (best < 0 || cache[i].first < cache[best].first)) best = (int)i;
        if (best >= 0) { void* p = cache[best].second; sizes.push_back({p, cache[best].first}); cache.erase(cache.begin() + best); return p; }
        size_t cap = 256;
        while (cap < bytes) cap += cap < (64u << 20) ? cap : (64u << 20);
        void* p = nullptr;
        if (hipMalloc(&p, cap) != hipSuccess) {
            // out of memory with blocks parked in the cache: give them back and try once more
            (void)hipGetLastError();
            for (auto& kv : cache) (void)hipFree(kv.second);
            cache.clear();
            if (hipMalloc(&p, cap) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        }
        sizes.push_back({p, cap});
        return p;
    }
    // parked blocks are bounded: consensus workspaces are tens of GB and their size differs from batch to batch, so the
    // oldest large blocks go back to the driver once the parked total passes the cap
    static constexpr size_t kCacheCap = (size_t)128 << 30;
    void release(void* p)
    {
        if (!p) return;
        std::lock_guard<std::mutex> g(mu);
        for (size_t i = 0; i < sizes.size(); ++i)
            if (sizes[i].first == p) {
                cache.push_back({sizes[i].second, p});
                sizes.erase(sizes.begin() + i);
                size_t parked = 0;
                for (auto& kv : cache) parked += kv.first;
                for (size_t k = 0; parked > kCacheCap && k < cache.size();) {
                    if (cache[k].first >= ((size_t)256 << 20)) { parked -= cache[k].first; (void)hipFree(cache[k].second); cache.erase(cache.begin() + k); }
                    else ++k;
                }
                return;
            }
    }
    std::vector<std::pair<void*, size_t>> sizes;   // live allocations
};

extern "C" clh_ctx* clh_create(int device)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) { fail(CLH_E_HIP, std::string("no HIP device: ") + hipGetErrorString(e)); return nullptr; }
    if (device < 0 || device >= n) { fail(CLH_E_ARG, "device index out of range"); return nullptr; }
    if ((e = hipSetDevice(device)) != hipSuccess) { fail(CLH_E_HIP, std::string("hipSetDevice: ") + hipGetErrorString(e)); return nullptr; }
    clh_ctx* c = new clh_ctx();
    c->device = device;
    { int v = 0; if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && v > 0) c->n_cu = v; }
    if ((e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess) {
        fail(CLH_E_HIP, std::string("hipStreamCreate: ") + hipGetErrorString(e));
        delete c;
        return nullptr;
    }
    bool ok = hipEventCreateWithFlags(&c->fork_ev, hipEventDisableTiming) == hipSuccess;
    for (int i = 0; i < 3 && ok; ++i)
        ok = hipStreamCreateWithFlags(&c->side[i], hipStreamNonBlocking) == hipSuccess &&
             hipEventCreateWithFlags(&c->join_ev[i], hipEventDisableTiming) == hipSuccess;
    if (!ok) { fail(CLH_E_HIP, "could not create side streams"); delete c; return nullptr; }
    return c;
}

extern "C" void clh_destroy(clh_ctx* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    for (auto& kv : c->cache) (void)hipFree(kv.second);
    for (auto& kv : c->sizes) (void)hipFree(kv.first);
    for (int i = 0; i < 3; ++i) { if (c->side[i]) (void)hipStreamDestroy(c->side[i]); if (c->join_ev[i]) (void)hipEventDestroy(c->join_ev[i]); }
    if (c->fork_ev) (void)hipEventDestroy(c->fork_ev);
    (void)hipStreamDestroy(c->stream);
    delete c;
}

extern "C" int clh_device_of(const clh_ctx* c) { return c ? c->device : -1; }

// What every plan kind and the resident genome share: the device blocks they take from the context's allocator and the
// events they create are recorded as they are handed out, and deleting the object gives all of them back.  Plans whose run is
// timed as a whole bracket it with begin_run / end_run, and their *_plan_timing reads elapsed.
struct clh_owned {
    clh_ctx* ctx = nullptr;
    bool ran = false;
    hipStream_t last_stream = nullptr;
    hipEvent_t run_ev[2] = {nullptr, nullptr};  // around the last run (created by the first)
    std::vector<void*> blocks;
    std::vector<hipEvent_t> events;

    explicit clh_owned(clh_ctx* c) : ctx(c) {}
    clh_owned(const clh_owned&) = delete;
    clh_owned& operator=(const clh_owned&) = delete;
    virtual ~clh_owned()
    {
        (void)hipSetDevice(ctx->device);
        if (ran) (void)hipStreamSynchronize(last_stream);
        for (void* b : blocks) ctx->release(b);
        for (hipEvent_t e : events) (void)hipEventDestroy(e);
    }
    void* alloc(size_t bytes)
    {
        void* p = ctx->alloc(bytes);
        if (p) blocks.push_back(p);
        return p;
    }
    // alloc + copy; null on failure (the block, if any, stays owned)
    void* upload(const void* host, size_t bytes)
    {
        void* p = alloc(bytes);
        return p && (bytes == 0 || hipMemcpy(p, host, bytes, hipMemcpyHostToDevice) == hipSuccess) ? p : nullptr;
    }
    // gives one block back before the object goes
    void free_block(void* p)
    {
        auto it = std::find(blocks.begin(), blocks.end(), p);
        if (it == blocks.end()) return;
        blocks.erase(it);
        ctx->release(p);
    }
    hipError_t event(hipEvent_t* e, unsigned flags = hipEventDefault)
    {
        const hipError_t r = hipEventCreateWithFlags(e, flags);
        if (r == hipSuccess) events.push_back(*e);
        return r;
    }
    // the start of a timed run: the device, the stream (the context's own unless one is given), the first event.  From here on
    // the destructor waits for the stream, whatever becomes of the launches that follow.
    int begin_run(void* stream_, hipStream_t* st)
    {
        HIPCHK(hipSetDevice(ctx->device));
        *st = stream_ ? (hipStream_t)stream_ : ctx->stream;
        if (!run_ev[0]) for (auto& e : run_ev) HIPCHK(event(&e));
        HIPCHK(hipEventRecord(run_ev[0], *st));
        last_stream = *st; ran = true;
        return 0;
    }
    int end_run()
    {
        HIPCHK(hipEventRecord(run_ev[1], last_stream));
        return 0;
    }
    int elapsed(float* ms)
    {
        HIPCHK(hipEventSynchronize(run_ev[1]));
        HIPCHK(hipEventElapsedTime(ms, run_ev[0], run_ev[1]));
        return 0;
    }
};

// ------------------------------------------------------------------------------------------------------------
// plan
// ------------------------------------------------------------------------------------------------------------
// The A/B switches of the Smith-Waterman classes, read once when a plan is built: the plan keeps them
struct SswSwitches {
    bool no_scan, no_scanw, no_slices, no_prefilter, no_lanes, no_pf2, no_tb_rows, no_guess, pf2_always;
    int pf2_share;
};

static SswSwitches ssw_switches()
{
    SswSwitches sw;
    sw.no_scan = getenv("CLH_NO_SCAN") != nullptr;
    sw.no_scanw = getenv("CLH_NO_SCANW") != nullptr;
    sw.no_slices = getenv("CLH_NO_SLICES") != nullptr;
    sw.no_prefilter = getenv("CLH_NO_PREFILTER") != nullptr;
    sw.no_lanes = getenv("CLH_NO_LANES") != nullptr;
    sw.no_pf2 = getenv("CLH_NO_PF2") != nullptr;
    sw.no_tb_rows = getenv("CLH_NO_TB_ROWS") != nullptr;
    sw.no_guess = getenv("CLH_NO_GUESS") != nullptr;
    sw.pf2_always = getenv("CLH_PF2_ALWAYS") != nullptr;
    const char* share = getenv("CLH_PF2_SHARE");
    sw.pf2_share = share ? std::max(1, atoi(share)) : 8;
    return sw;
}

struct clh_plan : clh_owned {
    using clh_owned::clh_owned;
    int n = 0;
    clh_ssw_opts opts;
    SswSwitches sw;
    clh::SswParams params;          // device pointers filled at run time
    bool quirk = false, do_cigar = false;
    std::vector<clh::SswTask> tasks;    // launch order
    struct Seg { int rv, begin, count; int64_t ws_off = 0; int ws_slot = 0, ws_wgs = 0; int lmax = 0; };      // ws_*: K1w classes, the workspaces of their persistent workgroups; lmax: K1a classes, longest read
    void* d_seg_ctr = nullptr;               // one work counter per segment
    std::vector<clh::ScanSlice> slices;      // window slices of the sliced scan class (one segment at most)
    void *d_slices = nullptr, *d_parts = nullptr;
    // the long-window classes behind the prefilter (ssw_prefilter.hip): [0] K1s (kRvScanSliced), [1] K1w (kRvScanWideSliced)
    struct PfClass {
        bool on = false;
        int ntasks = 0, nwork = 0, bpl = 0, cap = 0;
        void *d_win = nullptr, *d_pieces = nullptr, *d_work = nullptr, *d_dmin = nullptr, *d_queue = nullptr, *d_out = nullptr, *d_ctl = nullptr,
             *d_bound = nullptr, *d_parts = nullptr, *d_q2 = nullptr;
        int ws_row0 = 0, ws_slot = 0, ws_wgs = 0;
        int64_t ws_dirs_off = 0;
        int64_t extent = 0;                      // bytes of the refs buffer the kernel reads: the end of the last 256-byte block a window touches
        int64_t word_cols = 0, lane_insts = 0;   // the first stage's work: window columns x W words, and x (11 W + 8) instructions
        hipEvent_t ev[2] = {nullptr, nullptr};   // profiling runs: around ssw_prefilter_kernel
        bool timed = false;
    } pf[2];
    int n_rows = 0;                          // result rows: n_all + the scratch rows of the K1w long-window class
    std::vector<int32_t> slice_base;         // task-level slices of the anti-diagonal classes: first window column of scratch row k
    void* d_slice_base = nullptr;
    int n_all = 0;                           // tasks incl. those slices (their result rows sit behind the n real ones)
    std::vector<Seg> segs;
    void *d_tasks = nullptr, *d_results = nullptr, *d_colmax = nullptr, *d_cigars = nullptr, *d_cigar_len = nullptr,
         *d_pool = nullptr, *d_pool_head = nullptr;
    size_t colmax_elems = 0, cigar_elems = 0, strip_bytes = 0;
    unsigned long long pool_bytes = 0;
    void* d_strips = nullptr;
    hipEvent_t done_ev = nullptr;           // recorded behind the run's last launch: fetch waits for the RUN, not for what the caller queued later
    bool profiling = false;
    int64_t refs_bytes = -1;                 // size of the caller's refs buffer if stated (clh_plan_set_refs_bytes), else -1
    std::vector<hipEvent_t> ev;     // per segment: K1 start, K1 stop; then K1b small-window start/stop, large-window start/stop
    std::vector<int32_t> w32_prefix;   // tasks in launch order: how many before k could need the int32 traceback (clh::launch_traceback_w32)
    bool alpha = false;             // matrix edge 6..32: every alignment in the K1a classes (ssw_alpha.hip)
    void* d_alpha_mat = nullptr;    // their n x n matrix
    const void *run_reads = nullptr, *run_refs = nullptr;     // the last run's sequences (K1a's further traceback rounds in clh_ssw_fetch)

    // the workspaces of a class's persistent workgroups in the strip buffer: wgs slots of `bytes` rounded up to 256; returns their offset
    int64_t reserve_ws(size_t bytes, int wgs, int* slot)
    {
        *slot = (int)((bytes + 255) & ~(size_t)255);
        strip_bytes = (strip_bytes + 255) & ~(size_t)255;
        const int64_t off = (int64_t)strip_bytes;
        strip_bytes += (size_t)*slot * (size_t)wgs;
        return off;
    }
};

extern "C" void clh_plan_destroy(clh_plan* pl) { delete pl; }

// K1a (ssw_alpha.hip): the read-length bucket of an alignment over a matrix of edge 6..32
static int alpha_class_for(int64_t L)
{
    for (int b = 0; b < clh::kNumAlphaBuckets - 1; ++b)
        if (L <= clh::kAlphaRows[b]) return clh::kRvAlpha - b;
    return clh::kRvAlpha - (clh::kNumAlphaBuckets - 1);
}

static int rv_class_for(int64_t L)
{
    const int64_t rows = (L + 15) / 16 * 16;
    for (int i = 0; i < clh::kNumRvClasses; ++i)
        if (128 * clh::kRvClasses[i] >= rows) return clh::kRvClasses[i];
    return clh::kRvStrips;      // longer than 4096 rows: RV = 32 kernel with row strips
}

// K1s (ssw_scan.hip) takes the alignments whose scores provably fit the reference's 8-bit pass (ssw.c:804-806 chooses it and
// it cannot overflow), with the read short enough for its (score, row) keys and the gap extension for its 16-bit frames.
// CLH_NO_SCAN=1 in the environment sends everything to the anti-diagonal kernels (A/B measurements).
static bool scan_class_ok(int64_t L, const clh_ssw_opts* o, int max_match, int bias, const SswSwitches& sw)
{
    return !sw.no_scan && L <= 254 && o->score_size != 1 && (int64_t)max_match * L + bias < 255 && o->gap_extend >= 0 && o->gap_extend <= 16 && o->gap_open <= 255;
}

// K1w (ssw_scan_wide.hip): the same walk for what K1s leaves -- reads up to 4096 bases, any score below the 16-bit ceiling -- on
// windows that are not cut into slices.  CLH_NO_SCANW=1 switches it off (A/B measurements): the anti-diagonal classes take over.
static bool scanw_class_ok(int64_t L, int64_t R, const clh_ssw_opts* o, int max_match, const SswSwitches& sw)
{
    return !sw.no_scan && !sw.no_scanw && L <= 4096 && R < 32768 && (int64_t)max_match * L < 32000 && o->gap_extend >= 0 && o->gap_extend <= 16 && o->gap_open <= 255;
}

// K1s on long windows: the forward pass runs as slices of >= 8192 owned columns (at most 64 per alignment), each started
// `overlap` columns early (ssw_scan.hip: ssw_scan_slice_kernel).  Needs a positive gap extension (else a local alignment has
// no bounded span).  CLH_NO_SLICES=1 switches it off (A/B measurements).
static const int kSliceMinWindow = 32768, kSliceMinCols = 8192;
static bool scan_sliced(int64_t R, const clh_ssw_opts* o, const SswSwitches& sw)
{
    return !sw.no_slices && R >= kSliceMinWindow && o->gap_extend >= 1;
}

// The window slices of a long alignment: each owns `own` columns and starts `overlap` columns early -- a local alignment spans at
// most L (1 + max_match / gap_extend) columns (+ wildcard rows + slack).  At most 64 slices of >= 8192 owned columns, and with
// own_overlaps > 0 at least that many overlaps.
struct SliceGeom { int64_t overlap, own; };
static SliceGeom slice_geom(int64_t L, int64_t R, int max_match, int gap_extend, int own_overlaps)
{
    const int64_t overlap = L + (L * max_match + gap_extend - 1) / gap_extend + 32;
    return {overlap, std::max<int64_t>(std::max<int64_t>(kSliceMinCols, own_overlaps * overlap), (R + 63) / 64)};
}

// The sliced class behind the exact prefilter (ssw_prefilter.hip): needs the bound's constant c = min(max_match, gap_extend) >= 1
// and no second-best score (the column maxima of the columns it skips would be missing).  CLH_NO_PREFILTER=1 switches it off
// (A/B measurements, and the parity tests run both ways).
static bool prefilter_ok(const clh_ssw_opts* o, int max_match, const SswSwitches& sw)
{
    return !sw.no_prefilter && !o->want_score2 && max_match >= 1 && o->gap_extend >= 1;
}

// K1w on long windows (ssw_scan_wide.hip, class kRvScanWideSliced): what K1s's 8-bit class does not take, on windows of 32 kb and
// more with call-path options -- the prefilter in pieces of the read, a seed, candidate regions as K1w tasks.  Windows up to 1.5 Mb
// (a static slice + its overlap must stay inside K1w's 32 767 columns).  Without the prefilter (CLH_NO_PREFILTER) these alignments
// run as window-slice tasks of the anti-diagonal classes, as in rounds 2-3.
static bool scanw_sliced_ok(int64_t L, int64_t R, const clh_ssw_opts* o, int max_match, const SswSwitches& sw)
{
    if (sw.no_scan || sw.no_scanw || sw.no_slices || !prefilter_ok(o, max_match, sw)) return false;
    const SliceGeom g = slice_geom(L, R, max_match, o->gap_extend, 2);
    return L <= 4096 && R >= kSliceMinWindow && R <= 1500000 && g.own + g.overlap < 32768 && (int64_t)max_match * L < 32000 && o->gap_extend <= 16 && o->gap_open <= 255;
}

// K1l (ssw_lanes.hip): one alignment per lane for references of at most 64 columns -- the collapse stage's junction alignments
// (collapse.py:161-173, 251-256, 373-387).  Only where its plain recurrence IS what the reference computes: no second best (the column
// maxima of the reference's wildcard rows are not computed), gap_open > gap_extend or a score that cannot leave the 8-bit regime (the 16-bit
// pass with gap_open == gap_extend truncates F at stripe boundaries, rowmajor_spec.c), code 4 scoring 0.  A lane walks its alignment alone: a long
// read against a short reference goes there only when the plan holds enough of them to fill the GPU's lanes (`many`), else to the
// wave-per-alignment classes.  CLH_NO_LANES=1 switches the class off (A/B measurements, and the parity tests run both ways).
static int lanes_class_for(int64_t L, int64_t R, const clh_ssw_opts* o, int max_match, int bias, int null_code, bool many, const SswSwitches& sw)
{
    if (sw.no_lanes) return 0;
    if (o->want_score2 || R < 1 || R > 64 || L < 1 || L > 65535) return 0;
    if (!(o->n_mat <= 4 || null_code == 4)) return 0;
    if (o->gap_open > 255 || o->gap_extend < 0) return 0;
    if (o->gap_open <= o->gap_extend && !((int64_t)max_match * std::min(L, R) + bias < 255 && o->score_size != 1)) return 0;
    // a lane is alone with its alignment: ~25 ns per cell and pass.  Up to 2048 cells that is nothing; more only when the plan fills the GPU's lanes
    // (and then not beyond 262144 cells: a 6 ms chain)
    if ((!many && L * R > 2048) || L * R > 262144) return (L <= 32767 && !sw.no_scanw && !sw.no_scan) ? clh::kRvScanTr : 0;      // a wave per alignment, transposed (ssw_scan_wide.hip)
    return R <= 20 ? clh::kRvLanes20 : (R <= 32 ? clh::kRvLanes32 : (R <= 52 ? clh::kRvLanes52 : clh::kRvLanes64));
}

// the class of one alignment: K1a for the wide alphabets; else K1l / K1w-T, K1s (sliced on long windows), K1w, K1w behind the
// prefilter, the anti-diagonal classes by read length
static int ssw_class_for(int64_t L, int64_t R, const clh_ssw_opts* o, int max_match, int bias, int null_code, bool alpha, bool many,
                         const SswSwitches& sw)
{
    if (alpha) return alpha_class_for(L);
    if (int rv = lanes_class_for(L, R, o, max_match, bias, null_code, many, sw)) return rv;
    if (scan_class_ok(L, o, max_match, bias, sw)) return scan_sliced(R, o, sw) ? clh::kRvScanSliced : clh::kRvScan;
    if (scanw_class_ok(L, R, o, max_match, sw)) return clh::kRvScanWide;
    if (scanw_sliced_ok(L, R, o, max_match, sw)) return clh::kRvScanWideSliced;
    return rv_class_for(L);
}

// ref_off != nullptr: packed references, alignment a against [ref_off[a], ref_off[a+1]).  Otherwise windows of a resident
// genome: win_off[a], win_len[a], win_rc[a] (1 = read backwards and complemented).
static clh_plan* ssw_plan_build(clh_ctx* ctx, int32_t n, const int64_t* read_off, const int64_t* ref_off,
                                const int64_t* win_off, const int32_t* win_len, const uint8_t* win_rc,
                                const int32_t* mask_len, const clh_ssw_opts* o)
{
    if (!ctx || n < 0 || !read_off || (!ref_off && (!win_off || !win_len)) || !o || !o->mat) { fail(CLH_E_ARG, "clh_ssw_plan: null argument"); return nullptr; }
    if (o->n_mat < 1) { fail(CLH_E_UNSUPPORTED, "substitution matrix edge must be 1..32"); return nullptr; }
    if (o->gap_open < o->gap_extend) {
        fail(CLH_E_UNSUPPORTED, "gap_open < gap_extend: the reference's 8-bit lazy-F loop is not a plain recurrence there; not implemented");
        return nullptr;
    }
    if (o->n_mat > 32) { fail(CLH_E_UNSUPPORTED, "substitution matrix edge must be 1..32"); return nullptr; }
    // matrix edge 6..32 (protein alphabets): the K1a classes take every alignment; the resident genome is DNA
    const bool alpha = o->n_mat > 5;
    if (alpha && !ref_off) { fail(CLH_E_UNSUPPORTED, "windows of a resident genome take substitution matrices of edge 1..5 only"); return nullptr; }
    if (hipSetDevice(ctx->device) != hipSuccess) { fail(CLH_E_HIP, "hipSetDevice failed"); return nullptr; }
    clh_plan* pl = new clh_plan(ctx);
    pl->n = n; pl->opts = *o;
    const SswSwitches& sw = pl->sw = ssw_switches();
    clh::SswParams& P = pl->params;
    memset(&P, 0, sizeof(P));
    int mn = 0, mx = -128;
    for (int i = 0; i < o->n_mat * o->n_mat; ++i) { if (!alpha) P.mat[i] = o->mat[i]; mn = std::min(mn, (int)o->mat[i]); mx = std::max(mx, (int)o->mat[i]); }
    P.n = o->n_mat; P.gapO = o->gap_open; P.gapE = o->gap_extend; P.bias = -mn; P.max_match = mx; P.score_size = o->score_size;
    P.flag = o->flag; P.filters = o->filters; P.filterd = o->filterd;
    P.null_code = 5;
    if (o->n_mat == 5) {
        bool z = true;
        for (int i = 0; i < 5; ++i) z = z && o->mat[4 * 5 + i] == 0 && o->mat[i * 5 + 4] == 0;
        if (z) P.null_code = 4;
    }
    pl->opts.mat = nullptr;
    pl->alpha = alpha;
    pl->quirk = o->gap_open <= o->gap_extend;
    pl->do_cigar = o->want_cigar && (o->flag & 7) != 0;
    if (!(o->score_size == 0 || o->score_size == 1 || o->score_size == 2)) {
        fail(CLH_E_ARG, "Please call the function ssw_init before ssw_align.");   // ssw.c:818-821
        delete pl; return nullptr;
    }

    std::vector<int> cls(n);
    pl->tasks.resize(n);
    size_t colmax = 0, cig = 0;
    unsigned long long pool = 0;
    auto class_of = [&](int a, bool many) {
        const int64_t L = read_off[a + 1] - read_off[a], R = ref_off ? ref_off[a + 1] - ref_off[a] : (int64_t)win_len[a];
        return ssw_class_for(L, R, o, mx, -mn, P.null_code, alpha, many, sw);
    };
    int n_short_ref = 0;                     // alignments K1l could take: enough of them fill the GPU's lanes whatever their read length
    for (int a = 0; a < n; ++a) {
        const int rv = class_of(a, true);
        n_short_ref += clh::rv_is_lanes(rv) || rv == clh::kRvScanTr;
    }
    const bool many_short_ref = n_short_ref >= 32768;
    for (int a = 0; a < n; ++a) {
        const int64_t L = read_off[a + 1] - read_off[a], R = ref_off ? ref_off[a + 1] - ref_off[a] : (int64_t)win_len[a];
        if (L < 1 || R < 0 || L > 0x7fffffff || R > 0x7fffffff) { fail(CLH_E_ARG, "empty read or negative length in batch"); delete pl; return nullptr; }
        const int rc = (!ref_off && win_rc && win_rc[a]) ? 1 : 0;
        const int rv = class_of(a, many_short_ref);
        cls[a] = rv;
        clh::SswTask& t = pl->tasks[a];
        t.read_off = read_off[a]; t.ref_off = ref_off ? ref_off[a] : (rc ? win_off[a] + R - 1 : win_off[a]);
        t.ref_rc = rc; t.pad = 0;
        t.read_len = (int)L; t.ref_len = (int)R;
        t.mask_len = mask_len ? mask_len[a] : (L > 30 ? (int)(L / 2) : 15);
        t.out_index = a;
        t.colmax_off = (int64_t)colmax;
        if (o->want_score2) colmax += (size_t)((R + 7) & ~7ll);
        t.cigar_off = (int32_t)cig; t.cigar_cap = 0; t.dir_off = 0;
        if (rv == clh::kRvStrips) {     // two boundary buffers of (reference length rounded up to 64) x 8 bytes
            t.dir_off = (int64_t)pl->strip_bytes;
            pl->strip_bytes += 2 * (size_t)((R + 63) & ~63ll) * 8 + 256;
        }
        if (pl->do_cigar) {
            t.cigar_cap = (int32_t)(2 * L + 2);
            if (cig + (size_t)t.cigar_cap > 0x7fffffffull) { fail(CLH_E_CAPACITY, "batch too large for 32-bit CIGAR offsets; split it"); delete pl; return nullptr; }
            cig += (size_t)t.cigar_cap;
            // traceback workspace: the row kernel keeps 4 bits per cell of the band, 64 bytes per read row for bands up to
            // 128 cells, 128 up to 256 (ssw_traceback_rows.hip), of every iteration after the first (each twice the one
            // before); the few wide bands and the anti-diagonal kernel's per-iteration byte planes come out of the fixed slack added below
            pool += (unsigned long long)(L + 64) * 320ull;
        }
    }
    // Long windows of the anti-diagonal classes (reads outside K1s's 8-bit class), call-path options (no second best): the
    // alignment is cut into window slices that run as ordinary tasks of their class -- whole alignments of the read against
    // [c_begin, c_end), results into scratch rows behind the n real ones -- and a combining kernel (class kRvCombine, after
    // all classes have finished) takes the best slice: largest score, then smallest end column, then the earlier slice.
    // Exact: a local alignment spans at most L (1 + max_match / gap_extend) columns, so the slice that OWNS the end column
    // (started that far before its owned columns) computes the whole-window H there; a later slice that sees the same cell
    // in its overlap can only underestimate, and loses the tie.  The reverse pass of the owning slice runs inside the slice.
    int n_all = n;
    if (!alpha && !o->want_score2 && o->gap_extend >= 1 && !sw.no_slices) {
        for (int a = 0; a < n; ++a) {
            if (cls[a] < 1 || cls[a] == clh::kRvStrips || pl->tasks[a].ref_len < kSliceMinWindow) continue;
            const clh::SswTask par = pl->tasks[a];
            const int64_t R = par.ref_len;
            const auto [overlap, own] = slice_geom(par.read_len, R, mx, o->gap_extend, 2);
            const int rdir = par.ref_rc ? -1 : 1;
            pl->tasks[a].dir_off = (int64_t)pl->slice_base.size();       // first scratch row of this alignment (relative to n)
            int ns = 0;
            for (int64_t b = 0; b < R; b += own, ++ns) {
                clh::SswTask t = par;
                const int64_t cb = std::max<int64_t>(0, b - overlap), ce = std::min<int64_t>(R, b + own);
                t.ref_off = par.ref_off + cb * rdir; t.ref_len = (int32_t)(ce - cb);
                t.out_index = n + (int32_t)pl->slice_base.size();
                t.cigar_cap = 0; t.pad = 0; t.dir_off = 0;
                pl->slice_base.push_back((int32_t)cb);
                pl->tasks.push_back(t);
                cls.push_back(cls[a]);
            }
            pl->tasks[a].pad = ns;
            cls[a] = clh::kRvCombine;
        }
        n_all = (int)pl->tasks.size();
    }
    pl->n_all = n_all;
    P.n_real = n;
    pl->colmax_elems = colmax; pl->cigar_elems = cig;
    if (pl->do_cigar) pl->pool_bytes = std::min<unsigned long long>(pool + (1024ull << 20), 16ull << 30);

    // launch order: by row class, heaviest alignments first inside a class
    std::vector<int> order(n_all);
    for (int a = 0; a < n_all; ++a) order[a] = a;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) {
        if (cls[x] != cls[y]) return cls[x] < cls[y];
        const int64_t wx = (int64_t)pl->tasks[x].read_len * pl->tasks[x].ref_len, wy = (int64_t)pl->tasks[y].read_len * pl->tasks[y].ref_len;
        return wx > wy;
    });
    std::vector<clh::SswTask> sorted(n_all);
    for (int k = 0; k < n_all; ++k) sorted[k] = pl->tasks[order[k]];
    for (int k = 0; k < n_all;) {       // one segment per class
        int e = k;
        while (e < n_all && cls[order[e]] == cls[order[k]]) ++e;
        clh_plan::Seg sg; sg.rv = cls[order[k]]; sg.begin = k; sg.count = e - k;
        pl->segs.push_back(sg);
        k = e;
    }
    pl->tasks.swap(sorted);
    pl->n_rows = n_all;
    // the 16-bit traceback forms hand an alignment to the int32 one only if its score can reach 32767, its read + reference exceed
    // their LDS (12 352 bases) or its read their band ring (4 097 rows): classes without such a task skip that launch
    pl->w32_prefix.assign((size_t)n_all + 1, 0);
    for (int k = 0; k < n_all; ++k) {
        const clh::SswTask& t = pl->tasks[k];
        const bool maybe = t.out_index < n && ((int64_t)mx * t.read_len >= 32767 || (int64_t)t.read_len + t.ref_len > 12352 || t.read_len > 4097);
        pl->w32_prefix[k + 1] = pl->w32_prefix[k] + (maybe ? 1 : 0);
    }
    for (auto& sg : pl->segs) {
        if (sg.rv != clh::kRvScanWide && sg.rv != clh::kRvScanTr) continue;
        int lmax = 1;
        for (int k = 0; k < sg.count; ++k) lmax = std::max(lmax, sg.rv == clh::kRvScanTr ? 64 : (int)pl->tasks[sg.begin + k].read_len);
        sg.ws_wgs = std::min(sg.count, ctx->n_cu * 12);
        sg.ws_off = pl->reserve_ws(clh::scanw_task_bytes(lmax), sg.ws_wgs, &sg.ws_slot);
    }
    for (auto& sg : pl->segs) {
        if (!clh::rv_is_alpha(sg.rv)) continue;
        for (int k = 0; k < sg.count; ++k) sg.lmax = std::max(sg.lmax, (int)pl->tasks[sg.begin + k].read_len);
        if (sg.lmax <= clh::kAlphaLdsRows) continue;
        // the global form: pass state of the longest read per persistent workgroup
        sg.ws_wgs = std::min(sg.count, ctx->n_cu * 8);
        sg.ws_off = pl->reserve_ws(clh::alpha_lds_bytes(sg.lmax), sg.ws_wgs, &sg.ws_slot);
    }
    auto oom = [&] { fail(CLH_E_HIP, "out of device memory while building the plan"); delete pl; return nullptr; };
    if (alpha && !(pl->d_alpha_mat = pl->upload(o->mat, (size_t)o->n_mat * (size_t)o->n_mat))) return oom();
    if (!(pl->d_seg_ctr = pl->alloc(sizeof(int) * std::max<size_t>(pl->segs.size(), 1)))) return oom();
    for (const auto& sg : pl->segs) {
        const int ci = sg.rv == clh::kRvScanSliced ? 0 : (sg.rv == clh::kRvScanWideSliced ? 1 : -1);
        if (ci < 0 || !prefilter_ok(o, mx, sw)) continue;
        // per alignment: the 256-byte blocks of the refs buffer its window touches, in processing order (minus-strand windows run
        // down the addresses); per piece of its read (<= 254 rows) one run of block minima; a lane of the prefilter owns bpl blocks
        clh_plan::PfClass& f = pl->pf[ci];
        std::vector<clh::PfWin> wins(sg.count);
        std::vector<clh::PfTask> pieces;
        std::vector<clh::PfWork> work;
        int64_t total = 0, cap = 0, dtot = 0;
        int lmax = 1;
        for (int k = 0; k < sg.count; ++k) {
            const clh::SswTask& t = pl->tasks[sg.begin + k];
            clh::PfWin& w = wins[k];
            memset(&w, 0, sizeof(w));
            const int64_t R = t.ref_len;
            if (t.ref_rc) { const int64_t hi = t.ref_off, lo = hi - R + 1; w.mem_block0 = (int32_t)(hi >> 8); w.phase = (int32_t)(255 - (hi & 255)); w.nsub = (int32_t)((hi >> 8) - (lo >> 8) + 1); }
            else { const int64_t lo = t.ref_off, hi = lo + R - 1; w.mem_block0 = (int32_t)(lo >> 8); w.phase = (int32_t)(lo & 255); w.nsub = (int32_t)((hi >> 8) - (lo >> 8) + 1); }
            f.extent = std::max<int64_t>(f.extent, (((t.ref_rc ? t.ref_off : t.ref_off + R - 1) >> 8) + 1) << 8);
            const int L = t.read_len, K = (L + 253) / 254;
            w.piece_first = (int32_t)pieces.size(); w.piece_count = K; w.d_off = (int32_t)dtot;
            dtot += w.nsub;
            for (int q = 0, r0 = 0; q < K; ++q) {
                const int rows = L / K + (q < L % K ? 1 : 0);
                pieces.push_back({k, r0, rows, (int32_t)total});
                r0 += rows; total += w.nsub;
                const int64_t Wq = (rows + 31) / 32;
                f.word_cols += R * Wq; f.lane_insts += R * (11 * Wq + 8);
            }
            cap += ci == 0 ? std::max<int64_t>(64, w.nsub / 8 + 1) : 2 * 64;
            lmax = std::max(lmax, L);
            if (total > 0x7fffffffll || cap > 0x3fffffffll) { fail(CLH_E_CAPACITY, "batch too large for the prefilter's 32-bit block offsets; split it"); delete pl; return nullptr; }
        }
        const int bpl = (int)std::min<int64_t>(16, std::max<int64_t>(4, total / (64 * 12288)));
        for (int q = 0; q < (int)pieces.size(); ++q) {
            clh::PfWin& w = wins[pieces[q].task];
            if (q == w.piece_first) w.work_first = (int32_t)work.size();
            for (int fb = 0; fb < w.nsub; fb += 64 * bpl) work.push_back({q, fb});
            w.work_count = (int32_t)work.size() - w.work_first;
        }
        f.on = true; f.ntasks = sg.count; f.bpl = bpl; f.cap = (int)cap; f.nwork = (int)work.size();
        f.d_win = pl->upload(wins.data(), sizeof(clh::PfWin) * wins.size());
        f.d_pieces = pl->upload(pieces.data(), sizeof(clh::PfTask) * pieces.size());
        f.d_work = work.empty() ? pl->alloc(sizeof(clh::PfWork)) : pl->upload(work.data(), sizeof(clh::PfWork) * work.size());
        f.d_dmin = pl->alloc((size_t)total + 64);
        f.d_out = pl->alloc(sizeof(clh::PfOut) * wins.size());
        f.d_ctl = pl->alloc(sizeof(clh::PfCtl));
        if (!f.d_win || !f.d_pieces || !f.d_work || !f.d_dmin || !f.d_out || !f.d_ctl || hipMemset(f.d_ctl, 0, sizeof(clh::PfCtl)) != hipSuccess) return oom();
        if (ci == 0) {
            f.d_queue = pl->alloc(sizeof(clh::ScanSlice) * (size_t)cap);
            f.d_parts = pl->alloc(sizeof(clh::ScanPart) * (size_t)cap);
            if (!f.d_queue || !f.d_parts) return oom();
            // the second stage's queue: at most every entry of the work list (A/B: one stage only)
            if (!sw.no_pf2 && !(f.d_q2 = pl->alloc(sizeof(int32_t) * std::max<size_t>(work.size(), 1)))) return oom();
        } else {
            // 2 seed tasks per alignment in fixed places, then the candidate queue; 130 scratch result rows per alignment behind every other
            // row; the K1w workspaces belong to the persistent workgroups, not to the tasks
            f.d_queue = pl->alloc(sizeof(clh::WsTask) * ((size_t)2 * sg.count + (size_t)cap));
            f.d_bound = pl->alloc(sizeof(uint16_t) * (size_t)(dtot + 64));
            if (!f.d_queue || !f.d_bound) return oom();
            f.ws_row0 = pl->n_rows;
            pl->n_rows += clh::kWsRows * sg.count;
            f.ws_wgs = (int)std::min<int64_t>((int64_t)2 * sg.count + cap, (int64_t)ctx->n_cu * 12);
            f.ws_dirs_off = pl->reserve_ws(clh::scanw_task_bytes(lmax), f.ws_wgs, &f.ws_slot);
        }
    }
    for (const auto& sg : pl->segs) {
        if (sg.rv != clh::kRvScanSliced || pl->pf[0].on) continue;
        for (int k = 0; k < sg.count; ++k) {
            clh::SswTask& t = pl->tasks[sg.begin + k];
            const int64_t R = t.ref_len;
            const auto [overlap, own] = slice_geom(t.read_len, R, mx, o->gap_extend, 0);
            t.dir_off = (int64_t)pl->slices.size();
            int ns = 0;
            for (int64_t b = 0; b < R; b += own, ++ns) {
                clh::ScanSlice sl;
                memset(&sl, 0, sizeof(sl));
                sl.task = k; sl.own_begin = (int32_t)b; sl.c_begin = (int32_t)std::max<int64_t>(0, b - overlap); sl.c_end = (int32_t)std::min<int64_t>(R, b + own);
                sl.part = (int32_t)pl->slices.size();
                pl->slices.push_back(sl);
            }
            t.pad = ns;
        }
    }

    pl->d_tasks = n_all > 0 ? pl->upload(pl->tasks.data(), sizeof(clh::SswTask) * (size_t)n_all) : pl->alloc(sizeof(clh::SswTask));
    pl->d_results = pl->alloc(sizeof(clh::SswResult) * (size_t)std::max(pl->n_rows, 1));
    pl->d_cigar_len = pl->alloc(sizeof(int32_t) * (size_t)std::max(n_all, 1));
    if (!pl->d_tasks || !pl->d_results || !pl->d_cigar_len) return oom();
    if (!pl->slice_base.empty() && !(pl->d_slice_base = pl->upload(pl->slice_base.data(), sizeof(int32_t) * pl->slice_base.size()))) return oom();
    if (o->want_score2 && !(pl->d_colmax = pl->alloc(sizeof(uint16_t) * std::max<size_t>(colmax, 1)))) return oom();
    if (pl->do_cigar) {
        pl->d_cigars = pl->alloc(sizeof(uint32_t) * std::max<size_t>(cig, 1));
        pl->d_pool = pl->alloc((size_t)pl->pool_bytes);
        pl->d_pool_head = pl->alloc(clh::tb_head_bytes(n_all));
        if (!pl->d_cigars || !pl->d_pool || !pl->d_pool_head) return oom();
    }
    if (pl->strip_bytes && !(pl->d_strips = pl->alloc(pl->strip_bytes))) return oom();
    if (!pl->slices.empty()) {
        pl->d_slices = pl->upload(pl->slices.data(), sizeof(clh::ScanSlice) * pl->slices.size());
        pl->d_parts = pl->alloc(sizeof(clh::ScanPart) * pl->slices.size());
        if (!pl->d_slices || !pl->d_parts) return oom();
    }
    return pl;
}

extern "C" clh_plan* clh_ssw_plan(clh_ctx* ctx, int32_t n, const int64_t* read_off, const int64_t* ref_off,
                                  const int32_t* mask_len, const clh_ssw_opts* o)
{
    if (!ref_off) { fail(CLH_E_ARG, "clh_ssw_plan: null argument"); return nullptr; }
    return ssw_plan_build(ctx, n, read_off, ref_off, nullptr, nullptr, nullptr, mask_len, o);
}

extern "C" clh_plan* clh_ssw_plan_windows(clh_ctx* ctx, int32_t n, const int64_t* read_off, const int64_t* win_off, const int32_t* win_len,
                                          const uint8_t* win_rc, const int32_t* mask_len, const clh_ssw_opts* o)
{
    if (!win_off || !win_len) { fail(CLH_E_ARG, "clh_ssw_plan_windows: null argument"); return nullptr; }
    return ssw_plan_build(ctx, n, read_off, nullptr, win_off, win_len, win_rc, mask_len, o);
}

// ---------------------------------------------------------------------------------------------------------------
// K5: resident genome
// ---------------------------------------------------------------------------------------------------------------
struct clh_genome : clh_owned {
    using clh_owned::clh_owned;
    int64_t len = 0;
    void *d_codes = nullptr, *d_pre = nullptr;
    void* d_ascii = nullptr;                    // the characters themselves (K6 compares flanks as the reference's strings do)
    void* d_sites = nullptr;                    // annotated splice sites (K6): four sorted runs of int64 in one buffer
    int64_t n_sites[4] = {0, 0, 0, 0};
};

extern "C" void clh_genome_destroy(clh_genome* g) { delete g; }

extern "C" clh_genome* clh_genome_create(clh_ctx* ctx, const char* ascii, int64_t len)
{
    if (!ctx || len < 0 || (len > 0 && !ascii)) { fail(CLH_E_ARG, "clh_genome_create: null argument"); return nullptr; }
    if (hipSetDevice(ctx->device) != hipSuccess) { fail(CLH_E_HIP, "hipSetDevice failed"); return nullptr; }
    clh_genome* g = new clh_genome(ctx);
    g->len = len;
    const size_t nblk = (size_t)(len / clh::kGenomeBlock) + 2;
    g->d_codes = g->alloc((size_t)len + 64);
    g->d_pre = g->alloc(sizeof(unsigned int) * nblk);
    g->d_ascii = g->alloc((size_t)len + 64);
    void* d_ascii = g->d_ascii;
    bool ok = g->d_codes && g->d_pre && d_ascii;
    if (!ok) fail(CLH_E_HIP, "out of device memory for the genome");
    std::vector<unsigned int> pre(nblk, 0);
    if (ok && len > 0) {
        ok = hipMemsetAsync(g->d_pre, 0, sizeof(unsigned int) * nblk, ctx->stream) == hipSuccess &&
             hipMemcpyAsync(d_ascii, ascii, (size_t)len, hipMemcpyHostToDevice, ctx->stream) == hipSuccess &&
             clh::launch_genome_encode((const char*)d_ascii, (uint8_t*)g->d_codes, (unsigned int*)g->d_pre, len, ctx->stream) == hipSuccess &&
             hipMemcpyAsync(pre.data(), g->d_pre, sizeof(unsigned int) * nblk, hipMemcpyDeviceToHost, ctx->stream) == hipSuccess &&
             hipStreamSynchronize(ctx->stream) == hipSuccess;
        if (!ok) fail(CLH_E_HIP, "genome encode failed");
    }
    if (ok) {   // exclusive prefix: pre[b] = upper-case N before base b * kGenomeBlock
        unsigned int run = 0;
        for (size_t b = 0; b < nblk; ++b) { const unsigned int c = pre[b]; pre[b] = run; run += c; }
        ok = hipMemcpyAsync(g->d_pre, pre.data(), sizeof(unsigned int) * nblk, hipMemcpyHostToDevice, ctx->stream) == hipSuccess &&
             hipStreamSynchronize(ctx->stream) == hipSuccess;
        if (!ok) fail(CLH_E_HIP, "genome prefix upload failed");
    }
    if (!ok) { delete g; return nullptr; }
    return g;
}

extern "C" const void* clh_genome_codes(const clh_genome* g) { return g ? g->d_codes : nullptr; }
extern "C" int64_t clh_genome_length(const clh_genome* g) { return g ? g->len : 0; }

extern "C" int clh_genome_count_n(clh_genome* g, int32_t n, const int64_t* off, const int64_t* len, int64_t* out)
{
    if (!g || n < 0 || (n > 0 && (!off || !len || !out))) return fail(CLH_E_ARG, "clh_genome_count_n: null argument");
    if (n == 0) return 0;
    for (int i = 0; i < n; ++i) if (off[i] < 0 || len[i] < 0 || off[i] + len[i] > g->len) return fail(CLH_E_ARG, "clh_genome_count_n: window outside the genome");
    clh_ctx* ctx = g->ctx;
    HIPCHK(hipSetDevice(ctx->device));
    void* d_off = ctx->alloc(sizeof(int64_t) * (size_t)n); void* d_len = ctx->alloc(sizeof(int64_t) * (size_t)n); void* d_out = ctx->alloc(sizeof(int64_t) * (size_t)n);
    int rc = 0;
    if (!d_off || !d_len || !d_out) rc = fail(CLH_E_HIP, "out of device memory");
    if (!rc && (hipMemcpyAsync(d_off, off, sizeof(int64_t) * (size_t)n, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
                hipMemcpyAsync(d_len, len, sizeof(int64_t) * (size_t)n, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
                clh::launch_genome_count_n((const uint8_t*)g->d_codes, (const unsigned int*)g->d_pre, (const long long*)d_off, (const long long*)d_len,
                                           (long long*)d_out, n, ctx->stream) != hipSuccess ||
                hipMemcpyAsync(out, d_out, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
                hipStreamSynchronize(ctx->stream) != hipSuccess))
        rc = fail(CLH_E_HIP, "N count failed");
    if (rc) (void)hipStreamSynchronize(ctx->stream);      // nothing queued may still touch the buffers when they go back to the cache
    ctx->release(d_off); ctx->release(d_len); ctx->release(d_out);
    return rc;
}

// K6: annotated splice sites of the resident genome (the SS_INDEX of align.py:235-252, 275-316) as four sorted runs
extern "C" int clh_genome_set_splice_sites(clh_genome* g, const int64_t* pos, const int64_t* count4)
{
    if (!g || !count4) return fail(CLH_E_ARG, "clh_genome_set_splice_sites: null argument");
    int64_t tot = 0;
    for (int k = 0; k < 4; ++k) { if (count4[k] < 0) return fail(CLH_E_ARG, "clh_genome_set_splice_sites: negative count"); tot += count4[k]; }
    if (tot > 0 && !pos) return fail(CLH_E_ARG, "clh_genome_set_splice_sites: null argument");
    int64_t at = 0;
    for (int k = 0; k < 4; ++k) {
        for (int64_t i = 0; i < count4[k]; ++i) {
            const int64_t v = pos[at + i];
            if (v < 0 || v > g->len || (i > 0 && v <= pos[at + i - 1])) return fail(CLH_E_ARG, "clh_genome_set_splice_sites: positions must be strictly ascending and inside the genome");
        }
        at += count4[k];
    }
    clh_ctx* ctx = g->ctx;
    HIPCHK(hipSetDevice(ctx->device));
    g->free_block(g->d_sites); g->d_sites = nullptr;
    for (int k = 0; k < 4; ++k) g->n_sites[k] = 0;
    if (tot == 0) return 0;
    g->d_sites = g->alloc(sizeof(int64_t) * (size_t)tot);
    if (!g->d_sites) return fail(CLH_E_HIP, "out of device memory");
    if (hipMemcpyAsync(g->d_sites, pos, sizeof(int64_t) * (size_t)tot, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
        hipStreamSynchronize(ctx->stream) != hipSuccess) {
        g->free_block(g->d_sites); g->d_sites = nullptr;
        return fail(CLH_E_HIP, "splice-site upload failed");
    }
    for (int k = 0; k < 4; ++k) g->n_sites[k] = count4[k];
    return 0;
}

// K6: splice signals around n candidate junctions of the resident genome (align.py:474-733)
extern "C" int clh_splice_signal_batch(clh_genome* g, int32_t n, const int64_t* ctg_off, const int64_t* ctg_len, const int64_t* start,
                                       const int64_t* end, const int32_t* clip_base, const int32_t* host_mask, int32_t search_extra,
                                       int32_t shift_threshold, int32_t is_canonical, int32_t* out)
{
    if (!g || n < 0 || (n > 0 && (!ctg_off || !ctg_len || !start || !end || !clip_base || !host_mask || !out)))
        return fail(CLH_E_ARG, "clh_splice_signal_batch: null argument");
    if (n == 0) return 0;
    if (search_extra < 0 || shift_threshold < 0) return fail(CLH_E_ARG, "clh_splice_signal_batch: negative search length");
    std::vector<clh::SpliceTask> tasks((size_t)n);
    for (int i = 0; i < n; ++i) {
        if (ctg_off[i] < 0 || ctg_len[i] < 0 || ctg_off[i] + ctg_len[i] > g->len) return fail(CLH_E_ARG, "clh_splice_signal_batch: contig outside the genome");
        if (clip_base[i] < 0 || clip_base[i] > 4096) return fail(CLH_E_ARG, "clh_splice_signal_batch: clip_base out of range");
        if ((int64_t)clip_base[i] + search_extra > clh::kSpliceMaxSearch)     // the ranking key's fields would overflow (clh_device.h)
            return fail(CLH_E_ARG, "clh_splice_signal_batch: clip_base + search_extra above 16284");
        clh::SpliceTask& t = tasks[(size_t)i];
        t.ctg_off = ctg_off[i]; t.ctg_len = ctg_len[i]; t.start = start[i]; t.end = end[i]; t.clip_base = clip_base[i]; t.host_mask = host_mask[i];
    }
    clh_ctx* ctx = g->ctx;
    HIPCHK(hipSetDevice(ctx->device));
    const size_t tb = sizeof(clh::SpliceTask) * (size_t)n, ob = sizeof(int32_t) * 8 * (size_t)n;
    void* d_t = ctx->alloc(tb); void* d_o = ctx->alloc(ob);
    clh::SpliceSites sites;
    int64_t at = 0;
    for (int k = 0; k < 4; ++k) { sites.pos[k] = (const int64_t*)g->d_sites + at; sites.n[k] = g->n_sites[k]; at += g->n_sites[k]; }
    int rc = 0;
    if (!d_t || !d_o) rc = fail(CLH_E_HIP, "out of device memory");
    if (!rc && (hipMemcpyAsync(d_t, tasks.data(), tb, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
                clh::launch_splice_scan((const uint8_t*)g->d_codes, (const uint8_t*)g->d_ascii, (const clh::SpliceTask*)d_t, n, search_extra, shift_threshold, is_canonical & 3,
                                        sites, (int32_t*)d_o, ctx->stream) != hipSuccess ||
                hipMemcpyAsync(out, d_o, ob, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
                hipStreamSynchronize(ctx->stream) != hipSuccess))
        rc = fail(CLH_E_HIP, "splice-signal scan failed");
    if (rc) (void)hipStreamSynchronize(ctx->stream);      // see clh_genome_count_n
    ctx->release(d_t); ctx->release(d_o);
    return rc;
}

// Plans of one context may be in flight on the device at the same time (bench.py's C2 loop alternates two), but they share the context's
// side streams and fork/join events: clh_ssw_run must not be called from two host threads at once for plans of the same context.
extern "C" int clh_ssw_run(clh_plan* pl, const void* d_reads, const void* d_refs, void* stream_)
{
    if (!pl || !d_reads || !d_refs) return fail(CLH_E_ARG, "clh_ssw_run: null argument");
    HIPCHK(hipSetDevice(pl->ctx->device));
    hipStream_t st = stream_ ? (hipStream_t)stream_ : pl->ctx->stream;
    clh::SswParams P = pl->params;
    P.reads = (const int8_t*)d_reads; P.refs = (const int8_t*)d_refs;
    P.results = (clh::SswResult*)pl->d_results;
    P.colmax = (uint16_t*)pl->d_colmax;
    P.cigars = (uint32_t*)pl->d_cigars; P.cigar_len = (int32_t*)pl->d_cigar_len; P.dirs = (uint8_t*)pl->d_strips;
    P.no_guess = pl->sw.no_guess;
    pl->run_reads = d_reads; pl->run_refs = d_refs;
    if (pl->profiling && pl->ev.empty()) {
        pl->ev.resize(pl->segs.size() * 2 + 4);
        for (auto& e : pl->ev) HIPCHK(pl->event(&e));
    }
    // One launch per read-length class for K1, followed on the same stream by that class's small-window traceback.
    // Classes are independent, so outside profiling runs they go round-robin to the caller's stream and three side
    // streams (fork/join with events): the tail of one class overlaps the next, and the latency-bound traceback of
    // one class overlaps the VALU-bound score kernel of another.
    clh_ctx* c = pl->ctx;
    const bool tb = pl->do_cigar && pl->n > 0;
    const bool fan = !pl->profiling && pl->segs.size() > 1;
    const size_t eb = pl->segs.size() * 2;
    if (tb) HIPCHK(hipMemsetAsync(pl->d_pool_head, 0, 4 * 68, st));     // bump pointer and the classes' hand-over counters
    if (fan) {
        HIPCHK(hipEventRecord(c->fork_ev, st));
        for (int i = 0; i < 3; ++i) HIPCHK(hipStreamWaitEvent(c->side[i], c->fork_ev, 0));
    }
    // launch order: the class whose single alignments take longest first (a pass is a serial chain of reference columns,
    // longer per column the more rows a lane holds), the short-read scan class last: its many small workgroups would
    // otherwise fill every slot of the GPU and the long chains would start only when they drain
    std::vector<size_t> ord(pl->segs.size());
    for (size_t k = 0; k < ord.size(); ++k) ord[k] = k;
    std::sort(ord.begin(), ord.end(), [&](size_t x, size_t y) {
        auto weight = [](int rv) { return rv == clh::kRvStrips ? 1000 : (rv == clh::kRvScanWide ? 900 : (rv == clh::kRvScanWideSliced ? 800 : (rv == clh::kRvScanTr ? 700 : (clh::rv_is_alpha(rv) ? 600 + clh::kRvAlpha - rv : rv)))); };      // (K1w: whole long reads, one wave each; K1a: longest reads first)
        const int rx = weight(pl->segs[x].rv), ry = weight(pl->segs[y].rv);
        return rx > ry;
    });
    clh::SswParams PG = P;                                  // the traceback launches index the whole task table
    PG.tasks = (const clh::SswTask*)pl->d_tasks;
    uint8_t* const pool = (uint8_t*)pl->d_pool;
    unsigned long long* const head = (unsigned long long*)pl->d_pool_head;
    // CIGARs of one class, all on one stream: the row kernel, its wide form for what it hands over, the anti-diagonal
    // kernel for what is left (sized for the class; workgroups share the short lists).  Per class, so that the seconds-long
    // tail of a few wide-band alignments of one class runs under the score kernels of the others.
    auto traceback = [&](int first, int count, int seg, hipStream_t ls) -> int {
        // the anti-diagonal fallback stages both aligned sequences in LDS: always the largest configuration (12 kB of sequence,
        // 4098 rows) -- a short read can align against thousands of reference bases; its few workgroups share the list
        const int rvbig = 32;
        if (!pl->sw.no_tb_rows) {
            HIPCHK(clh::launch_traceback_rows(PG, first, count, pl->n_all, seg, pool, head, pl->pool_bytes, ls));
            HIPCHK(clh::launch_traceback_rows_wide(PG, first, count, pl->n_all, seg, pool, head, pl->pool_bytes, ls));
        } else HIPCHK(clh::launch_traceback_pool(0, PG, first, count, pl->n_all, seg, pool, head, pl->pool_bytes, ls));
        HIPCHK(clh::launch_traceback_pool(rvbig, PG, first, count, pl->n_all, seg, pool, head, pl->pool_bytes, ls));
        // what those 16-bit forms cannot hold (a score saturated at 32767, a sequence span or band past their LDS): int32 state
        if (pl->w32_prefix[first + count] > pl->w32_prefix[first]) HIPCHK(clh::launch_traceback_w32(PG, first, count, pool, head, pl->pool_bytes, ls));
        return 0;
    };
    // the first stage of the prefilter, with its own pair of events in profiling runs (clh_plan_prefilter_timing)
    auto prefilter = [&](clh_plan::PfClass& f, hipStream_t ls) -> int {
        f.timed = false;
        if (!P.pf_dmin) return 0;
        if (pl->profiling) {
            for (auto& e : f.ev) if (!e) HIPCHK(pl->event(&e));
            HIPCHK(hipEventRecord(f.ev[0], ls));
        }
        HIPCHK(clh::launch_ssw_prefilter(P, f.nwork, ls));
        if (pl->profiling) { HIPCHK(hipEventRecord(f.ev[1], ls)); f.timed = true; }
        return 0;
    };
    P.slice_base = (const int32_t*)pl->d_slice_base; PG.slice_base = P.slice_base;
    for (size_t q = 0; q < ord.size(); ++q) {
        const size_t k = ord[q];
        const auto& s = pl->segs[k];
        if (s.rv == clh::kRvCombine) continue;                   // after the join below: it reads the other classes' rows
        const hipStream_t ls = (fan && (q & 3)) ? c->side[(q & 3) - 1] : st;
        P.tasks = (const clh::SswTask*)pl->d_tasks + s.begin;
        if (pl->profiling) HIPCHK(hipEventRecord(pl->ev[2 * k + 0], ls));
        if ((s.rv == clh::kRvScanSliced && pl->pf[0].on) || s.rv == clh::kRvScanWideSliced) {
            // block minima of the bound, then seed + candidate slices (tasks), the slices, the finish -- one chain on the class's stream.
            // The prefilter reads the window text in address-aligned 256-byte blocks of the refs buffer: a buffer that is not
            // aligned so keeps the static slices (the pick kernels write them)
            clh_plan::PfClass& f = pl->pf[s.rv == clh::kRvScanSliced ? 0 : 1];
            P.pf_win = (const clh::PfWin*)f.d_win; P.pf_tasks = (const clh::PfTask*)f.d_pieces; P.pf_work = (const clh::PfWork*)f.d_work;
            P.pf_out = (clh::PfOut*)f.d_out; P.pf_ctl = (clh::PfCtl*)f.d_ctl; P.pf_bpl = f.bpl; P.pf_cap = f.cap;
            // ... nor does one whose stated size (clh_plan_set_refs_bytes) ends inside the last block a window touches
            P.pf_dmin = ((uintptr_t)d_refs & 255) == 0 && (pl->refs_bytes < 0 || f.extent <= pl->refs_bytes) ? (uint8_t*)f.d_dmin : nullptr;
            HIPCHK(hipMemsetAsync(f.d_ctl, 0, sizeof(clh::PfCtl), ls));
            if (s.rv == clh::kRvScanSliced) {
                P.pf_slices = (clh::ScanSlice*)f.d_queue; P.parts = (clh::ScanPart*)f.d_parts; P.pf_q2 = (int32_t*)f.d_q2; P.pf2_always = pl->sw.pf2_always; P.pf2_share = pl->sw.pf2_share;
                if (int rc = prefilter(f, ls)) return rc;
                HIPCHK(clh::launch_ssw_scan_filtered(pl->quirk, P, s.count, std::min(f.cap, c->n_cu * 12), std::min(f.nwork, c->n_cu * 16), ls));
            } else {
                P.ws_tasks = (clh::WsTask*)f.d_queue; P.ws_bound = (uint16_t*)f.d_bound; P.ws_row0 = f.ws_row0; P.ws_slot_bytes = f.ws_slot;
                P.ws_dirs_off = f.ws_dirs_off;
                if (int rc = prefilter(f, ls)) return rc;
                HIPCHK(clh::launch_ssw_scanw_filtered(pl->quirk, P, s.count, f.ws_wgs, P.pf_dmin != nullptr, ls));
            }
        } else if (s.rv == clh::kRvScanSliced) {
            P.slices = (const clh::ScanSlice*)pl->d_slices; P.parts = (clh::ScanPart*)pl->d_parts;
            HIPCHK(clh::launch_ssw_scan_sliced(pl->quirk, P, s.count, (int)pl->slices.size(), ls));
        } else if (clh::rv_is_alpha(s.rv)) HIPCHK(clh::launch_ssw_alpha(P, (const int8_t*)pl->d_alpha_mat, s.count, s.lmax, s.ws_wgs, (long long)s.ws_off, s.ws_slot, ls));
        else if (clh::rv_is_lanes(s.rv)) HIPCHK(clh::launch_ssw_lanes(clh::rv_lanes_columns(s.rv), P, s.count, ls));
        else if (s.rv == clh::kRvScan) HIPCHK(clh::launch_ssw_scan(pl->quirk, P, s.count, ls));
        else if (s.rv == clh::kRvScanTr) {
            int* ctr = (int*)pl->d_seg_ctr + k;
            HIPCHK(hipMemsetAsync(ctr, 0, sizeof(int), ls));
            HIPCHK(clh::launch_ssw_scanw_tr(pl->quirk, P, s.count, s.ws_wgs, ctr, (long long)s.ws_off, s.ws_slot, ls));
        }
        else if (s.rv == clh::kRvScanWide) {
            int* ctr = (int*)pl->d_seg_ctr + k;
            HIPCHK(hipMemsetAsync(ctr, 0, sizeof(int), ls));
            HIPCHK(clh::launch_ssw_scanw(pl->quirk, P, s.count, s.ws_wgs, ctr, (long long)s.ws_off, s.ws_slot, ls));
        }
        else HIPCHK(clh::launch_ssw(s.rv, pl->quirk, P, s.count, ls));
        if (pl->profiling) HIPCHK(hipEventRecord(pl->ev[2 * k + 1], ls));
        if (tb && !pl->profiling) {
            if (clh::rv_is_alpha(s.rv))
                HIPCHK(clh::launch_ssw_alpha_traceback(PG, (const int8_t*)pl->d_alpha_mat, s.begin, s.count, pl->n_all, (int)(k % clh::kTbMaxSeg), s.lmax,
                                                       pool, head, pl->pool_bytes, ls));
            else if (int rc = traceback(s.begin, s.count, (int)(k % clh::kTbMaxSeg), ls)) return rc;
        }
    }
    if (fan)
        for (int i = 0; i < 3; ++i) {
            HIPCHK(hipEventRecord(c->join_ev[i], c->side[i]));
            HIPCHK(hipStreamWaitEvent(st, c->join_ev[i], 0));
        }
    for (size_t k = 0; k < pl->segs.size(); ++k) {
        const auto& s = pl->segs[k];
        if (s.rv != clh::kRvCombine) continue;
        P.tasks = (const clh::SswTask*)pl->d_tasks + s.begin;
        if (pl->profiling) HIPCHK(hipEventRecord(pl->ev[2 * k + 0], st));
        HIPCHK(clh::launch_ssw_combine(P, s.count, st));
        if (pl->profiling) HIPCHK(hipEventRecord(pl->ev[2 * k + 1], st));
        if (tb && !pl->profiling) { if (int rc = traceback(s.begin, s.count, (int)(k % clh::kTbMaxSeg), st)) return rc; }
    }
    if (tb && pl->profiling && pl->alpha) {   // profiling runs of the K1a classes: their tracebacks after the score kernels, as one span
        HIPCHK(hipEventRecord(pl->ev[eb + 0], st));
        for (size_t k = 0; k < pl->segs.size(); ++k)
            HIPCHK(clh::launch_ssw_alpha_traceback(PG, (const int8_t*)pl->d_alpha_mat, pl->segs[k].begin, pl->segs[k].count, pl->n_all,
                                                   (int)(k % clh::kTbMaxSeg), pl->segs[k].lmax, pool, head, pl->pool_bytes, st));
        HIPCHK(hipEventRecord(pl->ev[eb + 1], st));
        HIPCHK(hipEventRecord(pl->ev[eb + 2], st));
        HIPCHK(hipEventRecord(pl->ev[eb + 3], st));
    } else if (tb && pl->profiling) {   // profiling runs: the traceback of all classes as serial launches after the score kernels
        const int rvmax = 32;
        HIPCHK(hipEventRecord(pl->ev[eb + 0], st));
        if (!pl->sw.no_tb_rows) HIPCHK(clh::launch_traceback_rows(PG, 0, pl->n_all, pl->n_all, 0, pool, head, pl->pool_bytes, st));
        else HIPCHK(clh::launch_traceback_pool(0, PG, 0, pl->n_all, pl->n_all, 0, pool, head, pl->pool_bytes, st));
        HIPCHK(hipEventRecord(pl->ev[eb + 1], st));
        HIPCHK(hipEventRecord(pl->ev[eb + 2], st));
        if (!pl->sw.no_tb_rows) HIPCHK(clh::launch_traceback_rows_wide(PG, 0, pl->n_all, pl->n_all, 0, pool, head, pl->pool_bytes, st));
        HIPCHK(clh::launch_traceback_pool(rvmax, PG, 0, pl->n_all, pl->n_all, 0, pool, head, pl->pool_bytes, st));
        HIPCHK(clh::launch_traceback_w32(PG, 0, pl->n_all, pool, head, pl->pool_bytes, st));
        HIPCHK(hipEventRecord(pl->ev[eb + 3], st));
    }
    if (!pl->done_ev) HIPCHK(pl->event(&pl->done_ev, hipEventDisableTiming));
    HIPCHK(hipEventRecord(pl->done_ev, st));
    pl->last_stream = st;
    pl->ran = true;
    return 0;
}

extern "C" int clh_plan_set_refs_bytes(clh_plan* pl, int64_t nbytes)
{
    if (!pl) return fail(CLH_E_ARG, "null plan");
    pl->refs_bytes = nbytes;
    return 0;
}

extern "C" int clh_plan_set_profiling(clh_plan* pl, int on)
{
    if (!pl) return fail(CLH_E_ARG, "null plan");
    pl->profiling = on != 0;
    return 0;
}

extern "C" int clh_plan_segments(const clh_plan* pl, int32_t cap, int32_t* rv, int32_t* count, int64_t* read_bases, int64_t* ref_bases)
{
    if (!pl) return fail(CLH_E_ARG, "null plan");
    const int ns = (int)pl->segs.size();
    for (int k = 0; k < ns && k < cap; ++k) {
        rv[k] = pl->segs[k].rv; count[k] = pl->segs[k].count;
        int64_t a = 0, b = 0;
        for (int t = pl->segs[k].begin; t < pl->segs[k].begin + pl->segs[k].count; ++t) { a += pl->tasks[t].read_len; b += pl->tasks[t].ref_len; }
        read_bases[k] = a; ref_bases[k] = b;
    }
    return ns;
}

// durations of the last run's launches, in ms (HIP events on the run's stream); waits for the run.
// k1_ms[segment]; k1b_ms[0] = small-window traceback launch (all alignments), k1b_ms[1] = large-window launches.
extern "C" int clh_plan_timing(clh_plan* pl, int32_t cap, float* k1_ms, float* k1b_ms)
{
    if (!pl || !pl->ran || !pl->profiling || pl->ev.empty()) return fail(CLH_E_ARG, "profiling was not enabled for the last run");
    HIPCHK(hipSetDevice(pl->ctx->device));
    HIPCHK(hipStreamSynchronize(pl->last_stream));
    const int ns = (int)pl->segs.size();
    for (int k = 0; k < ns && k < cap; ++k) HIPCHK(hipEventElapsedTime(&k1_ms[k], pl->ev[2 * k + 0], pl->ev[2 * k + 1]));
    k1b_ms[0] = k1b_ms[1] = 0.f;
    if (pl->do_cigar && pl->n > 0) {
        HIPCHK(hipEventElapsedTime(&k1b_ms[0], pl->ev[2 * ns + 0], pl->ev[2 * ns + 1]));   // small-window launch, all alignments
        HIPCHK(hipEventElapsedTime(&k1b_ms[1], pl->ev[2 * ns + 2], pl->ev[2 * ns + 3]));   // large-window launches, outliers only
    }
    return ns;
}

// counts[0] = alignments of the last run that the row traceback kernel handed to its wide form, counts[1] = alignments that
// went on to the anti-diagonal kernel (walks that leave the band, bands above 2048 cells); waits for the run
extern "C" int clh_plan_traceback_counts(clh_plan* pl, int32_t* counts)
{
    if (!pl || !counts || !pl->ran) return fail(CLH_E_ARG, "clh_plan_traceback_counts: no run yet");
    counts[0] = counts[1] = 0;
    if (!pl->d_pool_head) return 0;
    HIPCHK(hipSetDevice(pl->ctx->device));
    HIPCHK(hipStreamSynchronize(pl->last_stream));
    int32_t w[64];
    HIPCHK(hipMemcpy(w, (const char*)pl->d_pool_head + 16, sizeof(w), hipMemcpyDeviceToHost));
    for (int k = 0; k < 32; ++k) { counts[0] += w[k]; counts[1] += w[32 + k]; }
    return 0;
}

// what the prefilter of the sliced scan class did in the last run: out[0] alignments of the class, [1] of them with candidate
// slices instead of the static ones, [2] slices run, [3] window columns those slices computed, [4] window columns of the class;
// all zero when the plan has no such class or the filter is off; waits for the run
extern "C" int clh_plan_prefilter_stats(clh_plan* pl, int64_t* out)
{
    if (!pl || !out) return fail(CLH_E_ARG, "clh_plan_prefilter_stats: null argument");
    for (int k = 0; k < 6; ++k) out[k] = 0;
    if (!pl->ran) return 0;
    HIPCHK(hipSetDevice(pl->ctx->device));
    HIPCHK(hipStreamSynchronize(pl->last_stream));
    for (const auto& f : pl->pf) {
        if (!f.on) continue;
        clh::PfCtl c;
        HIPCHK(hipMemcpy(&c, f.d_ctl, sizeof(c), hipMemcpyDeviceToHost));
        out[0] += f.ntasks; out[1] += c.n_pruned; out[2] += c.qcount; out[3] += (int64_t)c.cols_scanned; out[4] += (int64_t)c.cols_window; out[5] += c.n_stage2;
    }
    return 0;
}

// ssw_prefilter_kernel alone in the last (profiling) run: ms[ci] = its duration for the K1s class (0) and the K1w class (1), 0 when it did
// not run; work[2 ci] = window columns x W words of the read's pieces, work[2 ci + 1] = the same columns x (11 W + 8), the kernel's
// instructions per column and lane -- what its issue-rate roofline counts
extern "C" int clh_plan_prefilter_timing(clh_plan* pl, float* ms, int64_t* work)
{
    if (!pl || !ms || !work) return fail(CLH_E_ARG, "clh_plan_prefilter_timing: null argument");
    if (!pl->ran || !pl->profiling) return fail(CLH_E_ARG, "profiling was not enabled for the last run");
    HIPCHK(hipSetDevice(pl->ctx->device));
    HIPCHK(hipStreamSynchronize(pl->last_stream));
    for (int ci = 0; ci < 2; ++ci) {
        const auto& f = pl->pf[ci];
        ms[ci] = 0.f; work[2 * ci] = work[2 * ci + 1] = 0;
        if (!f.on || !f.timed) continue;
        HIPCHK(hipEventElapsedTime(&ms[ci], f.ev[0], f.ev[1]));
        work[2 * ci] = f.word_cols; work[2 * ci + 1] = f.lane_insts;
    }
    return 0;
}

extern "C" const void* clh_ssw_results_dev(const clh_plan* pl) { return pl ? pl->d_results : nullptr; }

// CIGARs sit in worst-case shares (2 * readLen + 2 words per alignment, ~100x what is used): they are gathered into one
// dense run on the device and only that run crosses PCIe
__global__ void cigar_gather_kernel(const uint32_t* __restrict__ src, const int32_t* __restrict__ src_off, const int64_t* __restrict__ dst_off,
                                    const int32_t* __restrict__ len, uint32_t* __restrict__ dst)
{
    const int a = blockIdx.x, L = len[a];
    const uint32_t* s = src + src_off[a];
    uint32_t* d = dst + dst_off[a];
    for (int k = threadIdx.x; k < L; k += blockDim.x) d[k] = s[k];
}

// K1a's traceback keeps one byte per band cell of every band iteration in the pool, far more than the plan's share for an alignment
// whose band is wide: what did not fit in the run (CLH_STATUS_NEED_POOL) runs again here, over the emptied pool, in as many rounds as it
// takes (the scores are final).  A round in which none fits (several at once can fill the pool between them) is repeated one alignment
// after the other; there the first runs alone on the empty pool, and if it does not fit it is reported as CLH_ST_CIGAR_TRUNC.
static int alpha_pool_rounds(clh_plan* pl, std::vector<clh::SswResult>& res)
{
    const int n = pl->n;
    std::vector<int32_t> list(1, 0);
    for (int k = 0; k < pl->n_all; ++k) {
        const int a = pl->tasks[k].out_index;
        if (a < n && (res[a].status & clh::CLH_STATUS_NEED_POOL)) list.push_back(k);
    }
    if (list.size() == 1) return 0;
    clh_ctx* c = pl->ctx;
    hipStream_t st = c->stream;
    clh::SswParams PG = pl->params;
    PG.reads = (const int8_t*)pl->run_reads; PG.refs = (const int8_t*)pl->run_refs;
    PG.results = (clh::SswResult*)pl->d_results; PG.colmax = (uint16_t*)pl->d_colmax;
    PG.cigars = (uint32_t*)pl->d_cigars; PG.cigar_len = (int32_t*)pl->d_cigar_len; PG.dirs = (uint8_t*)pl->d_strips;
    PG.no_guess = pl->sw.no_guess;
    PG.tasks = (const clh::SswTask*)pl->d_tasks;
    void* d_list = c->alloc(sizeof(int32_t) * list.size());
    if (!d_list) return fail(CLH_E_HIP, "out of device memory for the traceback rounds");
    int rc = 0;
    bool one_by_one = false;
    while (list.size() > 1) {
        const int left = (int)list.size() - 1;
        list[0] = left;
        if (hipMemcpy(d_list, list.data(), sizeof(int32_t) * list.size(), hipMemcpyHostToDevice) != hipSuccess ||
            clh::launch_ssw_alpha_traceback_retry(PG, (const int8_t*)pl->d_alpha_mat, (int*)d_list, left, one_by_one, (uint8_t*)pl->d_pool,
                                                  (unsigned long long*)pl->d_pool_head, pl->pool_bytes, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess ||
            hipMemcpy(res.data(), pl->d_results, sizeof(clh::SswResult) * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess) {
            rc = fail(CLH_E_HIP, "traceback round failed");
            break;
        }
        std::vector<int32_t> next(1, 0);
        for (int q = 1; q <= left; ++q)
            if (res[pl->tasks[list[q]].out_index].status & clh::CLH_STATUS_NEED_POOL) next.push_back(list[q]);
        if ((int)next.size() - 1 == left) {      // not one of them fit
            if (!one_by_one) { one_by_one = true; continue; }
            // one by one, the first ran alone on the empty pool: it does not fit at all
            clh::SswResult& r = res[pl->tasks[list[1]].out_index];
            r.status = (r.status & ~clh::CLH_STATUS_NEED_POOL) | clh::CLH_STATUS_CIGAR_TRUNC;
            next.erase(next.begin() + 1);
            if (hipMemcpy(&((clh::SswResult*)pl->d_results)[pl->tasks[list[1]].out_index].status, &r.status, sizeof(r.status),
                          hipMemcpyHostToDevice) != hipSuccess) { rc = fail(CLH_E_HIP, "traceback round failed"); break; }
        }
        list.swap(next);
    }
    c->release(d_list);
    return rc;
}

extern "C" int clh_ssw_fetch(clh_plan* pl, clh_align_t* out, uint32_t* cigar_buf, int64_t cigar_cap, int64_t* cigar_used)
{
    if (!pl || !out) return fail(CLH_E_ARG, "clh_ssw_fetch: null argument");
    if (!pl->ran) return fail(CLH_E_ARG, "clh_ssw_fetch before clh_ssw_run");
    HIPCHK(hipSetDevice(pl->ctx->device));
    HIPCHK(pl->done_ev ? hipEventSynchronize(pl->done_ev) : hipStreamSynchronize(pl->last_stream));
    const int n = pl->n;
    std::vector<clh::SswResult> res((size_t)std::max(n, 1));
    std::vector<int32_t> clen((size_t)std::max(n, 1), 0);
    if (n > 0) HIPCHK(hipMemcpy(res.data(), pl->d_results, sizeof(clh::SswResult) * (size_t)n, hipMemcpyDeviceToHost));
    if (pl->alpha)
        for (int a = 0; a < n; ++a)
            if (res[a].status & clh::CLH_STATUS_BAD_CODE)
                return fail(CLH_E_ARG, "alignment " + std::to_string(a) + ": a read or reference code outside [0, " + std::to_string(pl->opts.n_mat) + ")");
    if (pl->alpha && pl->do_cigar && n > 0)
        if (int rc = alpha_pool_rounds(pl, res)) return rc;
    if (pl->do_cigar && n > 0) HIPCHK(hipMemcpy(clen.data(), pl->d_cigar_len, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost));
    std::vector<int32_t> share_off((size_t)std::max(n, 1), 0), glen((size_t)std::max(n, 1), 0);
    std::vector<int64_t> dst_off((size_t)std::max(n, 1), 0);
    for (const auto& t : pl->tasks) if (t.out_index < n) share_off[t.out_index] = t.cigar_off;
    int64_t used = 0;
    int rc = 0;
    for (int a = 0; a < n; ++a) {
        const clh::SswResult& r = res[a];
        clh_align_t& o = out[a];
        o.score1 = (uint16_t)r.score1; o.score2 = (uint16_t)r.score2;
        o.ref_begin1 = r.ref_begin1; o.ref_end1 = r.ref_end1; o.read_begin1 = r.read_begin1; o.read_end1 = r.read_end1;
        o.ref_end2 = r.ref_end2;
        o.status = 0;
        if (r.status & clh::CLH_STATUS_WORD) o.status |= CLH_ST_WORD;
        if (r.status & clh::CLH_STATUS_OVERFLOW8) o.status |= CLH_ST_NULL;
        if (r.status & clh::CLH_STATUS_TRACE_ERR) o.status |= CLH_ST_TRACE_ERR;
        if (r.status & clh::CLH_STATUS_NO_CIGAR) o.status |= CLH_ST_NO_CIGAR;
        if (r.status & clh::CLH_STATUS_CIGAR_TRUNC) o.status |= CLH_ST_CIGAR_TRUNC;
        o.cigar_off = -1; o.cigar_len = 0;
        if (!pl->do_cigar) { o.status |= CLH_ST_NO_CIGAR; continue; }
        const int len = clen[a];
        if (len > 0) {
            o.cigar_len = len;
            if (cigar_buf) {
                if (used + len > cigar_cap) { rc = CLH_E_CAPACITY; o.cigar_len = 0; continue; }
                o.cigar_off = (int32_t)used;
                dst_off[a] = used; glen[a] = len;
            }
            used += len;
        }
    }
    if (cigar_buf && pl->do_cigar && n > 0 && used > 0) {
        clh_ctx* c = pl->ctx;
        const size_t nb4 = sizeof(int32_t) * (size_t)n, nb8 = sizeof(int64_t) * (size_t)n;
        void *d_src = c->alloc(nb4), *d_len = c->alloc(nb4), *d_dst = c->alloc(nb8), *d_out = c->alloc(sizeof(uint32_t) * (size_t)used);
        int grc = 0;
        if (!d_src || !d_len || !d_dst || !d_out) grc = fail(CLH_E_HIP, "out of device memory while gathering CIGARs");
        hipStream_t st = c->stream;
        if (!grc && (hipMemcpyAsync(d_src, share_off.data(), nb4, hipMemcpyHostToDevice, st) != hipSuccess ||
                     hipMemcpyAsync(d_len, glen.data(), nb4, hipMemcpyHostToDevice, st) != hipSuccess ||
                     hipMemcpyAsync(d_dst, dst_off.data(), nb8, hipMemcpyHostToDevice, st) != hipSuccess)) grc = fail(CLH_E_HIP, "H2D failed");
        if (!grc) {
            hipLaunchKernelGGL(cigar_gather_kernel, dim3(n), dim3(64), 0, st, (const uint32_t*)pl->d_cigars, (const int32_t*)d_src, (const int64_t*)d_dst,
                               (const int32_t*)d_len, (uint32_t*)d_out);
            if (hipGetLastError() != hipSuccess) grc = fail(CLH_E_HIP, "cigar gather launch failed");
        }
        if (!grc && hipMemcpyAsync(cigar_buf, d_out, sizeof(uint32_t) * (size_t)used, hipMemcpyDeviceToHost, st) != hipSuccess) grc = fail(CLH_E_HIP, "D2H failed");
        const hipError_t se = hipStreamSynchronize(st);      // also before the buffers go back to the cache
        if (!grc && se != hipSuccess) grc = fail(CLH_E_HIP, "cigar gather failed");
        c->release(d_src); c->release(d_len); c->release(d_dst); c->release(d_out);
        if (grc) return grc;
    }
    if (cigar_used) *cigar_used = used;
    if (rc) return fail(rc, "cigar buffer too small");
    return 0;
}

extern "C" int clh_ssw_batch(clh_ctx* ctx, int32_t n, const int8_t* reads, const int64_t* read_off, const int8_t* refs,
                             const int64_t* ref_off, const int32_t* mask_len, const clh_ssw_opts* opts, clh_align_t* out,
                             uint32_t* cigar_buf, int64_t cigar_cap, int64_t* cigar_used)
{
    if (!ctx || !reads || !refs || !read_off || !ref_off) return fail(CLH_E_ARG, "clh_ssw_batch: null argument");
    clh_plan* pl = clh_ssw_plan(ctx, n, read_off, ref_off, mask_len, opts);
    if (!pl) return g_code;
    int rc = 0;
    if (pl->alpha) {       // codes outside the matrix: named here, before anything runs (the kernel checks them too)
        const int nm = pl->opts.n_mat;
        for (int a = 0; a < n && !rc; ++a) {
            bool bad = false;
            for (int64_t k = read_off[a]; k < read_off[a + 1] && !bad; ++k) bad = reads[k] < 0 || reads[k] >= nm;
            for (int64_t k = ref_off[a]; k < ref_off[a + 1] && !bad; ++k) bad = refs[k] < 0 || refs[k] >= nm;
            if (bad) rc = fail(CLH_E_ARG, "alignment " + std::to_string(a) + ": a read or reference code outside [0, " + std::to_string(nm) + ")");
        }
        if (rc) { delete pl; return rc; }
    }
    const size_t rb = (size_t)read_off[n], fb = (size_t)ref_off[n];
    void* d_reads = pl->alloc(rb + 64);
    void* d_refs = pl->alloc(fb + 64);
    if (!d_reads || !d_refs) { rc = fail(CLH_E_HIP, "out of device memory for the batch"); }
    if (!rc && hipMemcpyAsync(d_reads, reads, rb, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) rc = fail(CLH_E_HIP, "H2D reads failed");
    if (!rc && hipMemcpyAsync(d_refs, refs, fb, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) rc = fail(CLH_E_HIP, "H2D refs failed");
    if (!rc) rc = clh_ssw_run(pl, d_reads, d_refs, nullptr);
    if (!rc) rc = clh_ssw_fetch(pl, out, cigar_buf, cigar_cap, cigar_used);
    delete pl;
    return rc;
}

// clh_ssw_batch with the references given as windows of a resident genome: only the reads cross PCIe
extern "C" int clh_ssw_windows_batch(clh_genome* genome, int32_t n, const int8_t* reads, const int64_t* read_off, const int64_t* win_off,
                                     const int32_t* win_len, const uint8_t* win_rc, const int32_t* mask_len, const clh_ssw_opts* opts,
                                     clh_align_t* out, uint32_t* cigar_buf, int64_t cigar_cap, int64_t* cigar_used)
{
    if (!genome || !reads || !read_off || !win_off || !win_len) return fail(CLH_E_ARG, "clh_ssw_windows_batch: null argument");
    for (int i = 0; i < n; ++i)
        if (win_off[i] < 0 || win_len[i] < 0 || win_off[i] + win_len[i] > genome->len) return fail(CLH_E_ARG, "clh_ssw_windows_batch: window outside the genome");
    clh_ctx* ctx = genome->ctx;
    clh_plan* pl = clh_ssw_plan_windows(ctx, n, read_off, win_off, win_len, win_rc, mask_len, opts);
    if (!pl) return g_code;
    int rc = 0;
    const size_t rb = (size_t)read_off[n];
    void* d_reads = pl->alloc(rb + 64);
    if (!d_reads) { rc = fail(CLH_E_HIP, "out of device memory for the batch"); }
    if (!rc && hipMemcpyAsync(d_reads, reads, rb, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) rc = fail(CLH_E_HIP, "H2D reads failed");
    if (!rc) rc = clh_ssw_run(pl, d_reads, genome->d_codes, nullptr);
    if (!rc) rc = clh_ssw_fetch(pl, out, cigar_buf, cigar_cap, cigar_used);
    delete pl;
    return rc;
}

// ---------------------------------------------------------------------------------------------------------------
// K4: unit-cost edit distance of n pairs of byte strings (utils.py:153-159 `distance`)
// ---------------------------------------------------------------------------------------------------------------
struct clh_edit_plan : clh_owned {
    using clh_owned::clh_owned;
    int n = 0, planes = 3;
    std::vector<clh::EdTask> tasks;          // launch order (by lane-group class, longest text first)
    std::vector<int32_t> trivial;            // out[k] for pairs with an empty side, -1 otherwise
    void *d_sym = nullptr, *d_tasks = nullptr, *d_out = nullptr, *d_carry = nullptr;
};

static int ed_group(const clh::EdTask& t) { int B = (t.pat_len + 63) >> 6, G = 1; while (G < B && G < 64) G <<= 1; return G; }   // above 64 blocks: passes

extern "C" void clh_edit_plan_destroy(clh_edit_plan* pl) { delete pl; }

// uploads the strings (as dense symbol codes) and the task table; the plan then runs any number of times
extern "C" clh_edit_plan* clh_edit_plan_create(clh_ctx* ctx, int32_t n, const uint8_t* a, const int64_t* a_off, const uint8_t* b, const int64_t* b_off)
{
    if (!ctx || n < 0 || !a_off || !b_off || (n > 0 && (!a || !b))) { fail(CLH_E_ARG, "clh_edit_plan_create: null argument"); return nullptr; }
    if (hipSetDevice(ctx->device) != hipSuccess) { fail(CLH_E_HIP, "hipSetDevice failed"); return nullptr; }
    const int64_t ta = n ? a_off[n] - a_off[0] : 0, tb = n ? b_off[n] - b_off[0] : 0;
    if (ta < 0 || tb < 0) { fail(CLH_E_ARG, "clh_edit_plan_create: offsets must ascend"); return nullptr; }
    clh_edit_plan* pl = new clh_edit_plan(ctx);
    pl->n = n;
    // the batch's alphabet -> dense codes; the kernel builds match vectors from 3 bit planes (<= 8 symbols: DNA) or 8
    int code[256];
    for (int& c : code) c = -1;
    int nsym = 0;
    auto learn = [&](const uint8_t* p, int64_t len) { for (int64_t i = 0; i < len; ++i) if (code[p[i]] < 0) code[p[i]] = nsym++; };
    if (n) { learn(a + a_off[0], ta); learn(b + b_off[0], tb); }
    pl->planes = nsym <= 8 ? 3 : 8;
    std::vector<uint8_t> sym((size_t)(ta + tb) + 32, 0);
    for (int64_t i = 0; i < ta; ++i) sym[(size_t)i] = (uint8_t)code[a[a_off[0] + i]];
    for (int64_t i = 0; i < tb; ++i) sym[(size_t)(ta + i)] = (uint8_t)code[b[b_off[0] + i]];
    pl->trivial.assign((size_t)n, -1);
    pl->tasks.reserve((size_t)n);
    size_t carry_bytes = 0;
    for (int k = 0; k < n; ++k) {
        const int64_t la = a_off[k + 1] - a_off[k], lb = b_off[k + 1] - b_off[k];
        if (la < 0 || lb < 0) { fail(CLH_E_ARG, "clh_edit_plan_create: offsets must ascend"); delete pl; return nullptr; }
        if (la == 0 || lb == 0) { pl->trivial[(size_t)k] = (int32_t)(la + lb); continue; }
        clh::EdTask t;
        const bool a_is_pat = la <= lb;
        t.pat_off = a_is_pat ? a_off[k] - a_off[0] : ta + (b_off[k] - b_off[0]);
        t.txt_off = a_is_pat ? ta + (b_off[k] - b_off[0]) : a_off[k] - a_off[0];
        t.pat_len = (int32_t)(a_is_pat ? la : lb); t.txt_len = (int32_t)(a_is_pat ? lb : la);
        t.out_index = k; t.carry_off64 = -1;
        if (t.pat_len > 4096) {      // swept in passes of 64 blocks: two buffers of one byte per text column (+ slack for 16-byte reads)
            t.carry_off64 = (int32_t)(carry_bytes / 64);
            carry_bytes += 2 * ((((size_t)t.txt_len + 63) & ~(size_t)63) + 64);
        }
        pl->tasks.push_back(t);
    }
    std::stable_sort(pl->tasks.begin(), pl->tasks.end(), [&](const clh::EdTask& x, const clh::EdTask& y) {
        const int gx = ed_group(x), gy = ed_group(y);
        if (gx != gy) return gx < gy;
        return x.txt_len > y.txt_len;                 // similar step counts share a wave
    });
    const size_t nt = pl->tasks.size();
    pl->d_sym = pl->upload(sym.data(), sym.size());
    pl->d_tasks = nt ? pl->upload(pl->tasks.data(), sizeof(clh::EdTask) * nt) : pl->alloc(sizeof(clh::EdTask));
    pl->d_out = pl->alloc(sizeof(int32_t) * (size_t)std::max(n, 1));
    if (carry_bytes) pl->d_carry = pl->alloc(carry_bytes + 64);
    if (!pl->d_sym || !pl->d_tasks || !pl->d_out || (carry_bytes && !pl->d_carry)) {
        fail(CLH_E_HIP, "out of device memory or upload failed while building the edit-distance plan");
        delete pl; return nullptr;
    }
    return pl;
}

extern "C" int clh_edit_plan_run(clh_edit_plan* pl, void* stream_)
{
    if (!pl) return fail(CLH_E_ARG, "clh_edit_plan_run: null argument");
    hipStream_t st;
    if (int rc = pl->begin_run(stream_, &st)) return rc;
    const int nt = (int)pl->tasks.size();
    for (int i = 0; i < nt;) {
        const int G = ed_group(pl->tasks[(size_t)i]);
        int j = i;
        while (j < nt && ed_group(pl->tasks[(size_t)j]) == G) ++j;
        HIPCHK(clh::launch_edit_distance((const uint8_t*)pl->d_sym, (const clh::EdTask*)pl->d_tasks + i, j - i, G, pl->planes, (int32_t*)pl->d_out, (int8_t*)pl->d_carry, st));
        i = j;
    }
    return pl->end_run();
}

extern "C" int clh_edit_plan_fetch(clh_edit_plan* pl, int32_t* out)
{
    if (!pl || !out) return fail(CLH_E_ARG, "clh_edit_plan_fetch: null argument");
    if (!pl->ran) return fail(CLH_E_ARG, "clh_edit_plan_fetch before clh_edit_plan_run");
    HIPCHK(hipSetDevice(pl->ctx->device));
    HIPCHK(hipStreamSynchronize(pl->last_stream));
    std::vector<int32_t> res((size_t)std::max(pl->n, 1));
    if (pl->n) HIPCHK(hipMemcpy(res.data(), pl->d_out, sizeof(int32_t) * (size_t)pl->n, hipMemcpyDeviceToHost));
    for (int k = 0; k < pl->n; ++k) out[k] = pl->trivial[(size_t)k] >= 0 ? pl->trivial[(size_t)k] : res[(size_t)k];
    return 0;
}

extern "C" int clh_edit_plan_timing(clh_edit_plan* pl, float* ms)
{
    if (!pl || !ms || !pl->ran) return fail(CLH_E_ARG, "clh_edit_plan_timing: no run to time");
    return pl->elapsed(ms);
}

extern "C" int clh_edit_distance_batch(clh_ctx* ctx, int32_t n, const uint8_t* a, const int64_t* a_off, const uint8_t* b, const int64_t* b_off,
                                       int32_t* out)
{
    if (!out) return fail(CLH_E_ARG, "clh_edit_distance_batch: null argument");
    if (n == 0) return 0;
    clh_edit_plan* pl = clh_edit_plan_create(ctx, n, a, a_off, b, b_off);
    if (!pl) return g_code;
    int rc = clh_edit_plan_run(pl, nullptr);
    if (!rc) rc = clh_edit_plan_fetch(pl, out);
    delete pl;
    return rc;
}

// ---------------------------------------------------------------------------------------------------------------
// K4 on whole groups: strings uploaded once, compression and the pair tasks built on the device (edit_matrix.hip)
// ---------------------------------------------------------------------------------------------------------------
struct clh_edit_matrix_plan : clh_owned {
    using clh_owned::clh_owned;
    int nseq = 0, ngroups = 0, planes = 3;
    bool hpc = false;
    int64_t npairs = 0, total = 0, carry_cap64 = 0;
    uint8_t letter[256] = {0};                 // dense code -> the caller's byte
    std::vector<int64_t> seq_off;              // [nseq + 1], from 0
    std::vector<int32_t> len;                  // [nseq]: raw lengths, after a run with compression the compressed ones
    clh::EmCtl ctl;                            // as the last run left it
    void *d_raw = nullptr, *d_hpc = nullptr, *d_seq_off = nullptr, *d_len = nullptr, *d_group_off = nullptr, *d_pair_base = nullptr;
    void *d_tasks = nullptr, *d_out = nullptr, *d_ctl = nullptr, *d_carry = nullptr;
};

extern "C" void clh_edit_matrix_plan_destroy(clh_edit_matrix_plan* pl) { delete pl; }

extern "C" clh_edit_matrix_plan* clh_edit_matrix_plan_create(clh_ctx* ctx, int32_t nseq, const uint8_t* seqs, const int64_t* seq_off, int32_t ngroups,
                                                             const int64_t* group_off, int32_t flags)
{
    const char* me = "clh_edit_matrix_plan_create: ";
    if (!ctx || nseq < 0 || ngroups < 0 || !seq_off || (ngroups > 0 && !group_off) || (flags & ~CLH_EM_HPC)) { fail(CLH_E_ARG, std::string(me) + "bad argument"); return nullptr; }
    for (int s = 0; s < nseq; ++s) {
        const int64_t l = seq_off[s + 1] - seq_off[s];
        if (l < 0) { fail(CLH_E_ARG, std::string(me) + "offsets must ascend"); return nullptr; }
        if (l > INT32_MAX) { fail(CLH_E_ARG, std::string(me) + "a string of 2^31 bytes or more"); return nullptr; }
    }
    const int64_t total = seq_off[nseq] - seq_off[0];
    if (total > 0 && !seqs) { fail(CLH_E_ARG, std::string(me) + "null argument"); return nullptr; }
    std::vector<int64_t> pair_base((size_t)ngroups + 1, 0);
    for (int g = 0; g < ngroups; ++g) {
        const int64_t m = group_off[g + 1] - group_off[g];
        if (m < 0 || group_off[g] < 0 || group_off[g + 1] > nseq) { fail(CLH_E_ARG, std::string(me) + "group offsets must ascend within 0..nseq"); return nullptr; }
        if (m > 65536 || pair_base[(size_t)g] + m * (m - 1) / 2 > INT32_MAX) {
            fail(CLH_E_CAPACITY, std::string(me) + "more than 2^31 - 1 pairs"); return nullptr;
        }
        pair_base[(size_t)g + 1] = pair_base[(size_t)g] + m * (m - 1) / 2;
    }
    if (hipSetDevice(ctx->device) != hipSuccess) { fail(CLH_E_HIP, "hipSetDevice failed"); return nullptr; }
    clh_edit_matrix_plan* pl = new clh_edit_matrix_plan(ctx);
    pl->nseq = nseq; pl->ngroups = ngroups; pl->hpc = (flags & CLH_EM_HPC) != 0;
    pl->npairs = pair_base[(size_t)ngroups]; pl->total = total;
    // the batch's alphabet -> dense codes, as clh_edit_plan_create does (compression keeps the set of letters)
    int code[256];
    for (int& c : code) c = -1;
    int nsym = 0;
    const uint8_t* src = seqs + seq_off[0];
    std::vector<uint8_t> sym((size_t)total + 32, 0);
    for (int64_t i = 0; i < total; ++i) {
        const uint8_t c = src[i];
        if (code[c] < 0) { pl->letter[nsym] = c; code[c] = nsym++; }
        sym[(size_t)i] = (uint8_t)code[c];
    }
    pl->planes = nsym <= 8 ? 3 : 8;
    pl->seq_off.resize((size_t)nseq + 1);
    pl->len.resize((size_t)nseq);
    for (int s = 0; s <= nseq; ++s) pl->seq_off[(size_t)s] = seq_off[s] - seq_off[0];
    for (int s = 0; s < nseq; ++s) pl->len[(size_t)s] = (int32_t)(seq_off[s + 1] - seq_off[s]);
    // between-pass delta space of K4 for patterns above 4096 symbols: sized from the raw lengths, which bound the compressed ones.
    // Per group, the strings above 4096 in ascending order: the r-th is the text of its r pairs with shorter ones.
    unsigned long long carry64 = 0;
    std::vector<int32_t> longs;
    for (int g = 0; g < ngroups; ++g) {
        longs.clear();
        for (int64_t s = group_off[g]; s < group_off[g + 1]; ++s) if (pl->len[(size_t)s] > 4096) longs.push_back(pl->len[(size_t)s]);
        std::sort(longs.begin(), longs.end());
        for (size_t r = 1; r < longs.size(); ++r) carry64 += (unsigned long long)r * 2ull * (((unsigned long long)longs[r] + 63) / 64 + 1);
    }
    if (const char* e = getenv("CLH_EM_CARRY_BYTES")) carry64 = std::min<unsigned long long>(carry64, strtoull(e, nullptr, 10) / 64);   // tests: too little of it (the run fails)
    if (carry64 > (unsigned long long)INT32_MAX) { fail(CLH_E_CAPACITY, std::string(me) + "the pairs of strings above 4096 bytes need more than 128 GiB between passes"); delete pl; return nullptr; }
    pl->carry_cap64 = (int64_t)carry64;
    const size_t np = (size_t)std::max<int64_t>(pl->npairs, 1);
    std::vector<int64_t> goff((size_t)ngroups + 1, 0);
    for (int g = 0; g <= ngroups && ngroups > 0; ++g) goff[(size_t)g] = group_off[g];
    pl->d_raw = pl->upload(sym.data(), sym.size());
    pl->d_seq_off = pl->upload(pl->seq_off.data(), sizeof(int64_t) * pl->seq_off.size());
    pl->d_len = pl->alloc(sizeof(int32_t) * (size_t)std::max(nseq, 1));
    pl->d_group_off = pl->upload(goff.data(), sizeof(int64_t) * goff.size());
    pl->d_pair_base = pl->upload(pair_base.data(), sizeof(int64_t) * pair_base.size());
    pl->d_tasks = pl->alloc(sizeof(clh::EdTask) * np);
    pl->d_out = pl->alloc(sizeof(int32_t) * np);
    pl->d_ctl = pl->alloc(sizeof(clh::EmCtl));
    bool ok = pl->d_raw && pl->d_seq_off && pl->d_len && pl->d_group_off && pl->d_pair_base && pl->d_tasks && pl->d_out && pl->d_ctl;
    if (ok && pl->hpc) {
        // K4 reads text 16 bytes at a time past a string's end: the compressed buffer carries the same slack, zeroed once
        pl->d_hpc = pl->alloc(sym.size());
        ok = pl->d_hpc && hipMemset(pl->d_hpc, 0, sym.size()) == hipSuccess;
    }
    if (ok && !pl->hpc && nseq) ok = hipMemcpy(pl->d_len, pl->len.data(), sizeof(int32_t) * (size_t)nseq, hipMemcpyHostToDevice) == hipSuccess;
    if (ok && carry64) { pl->d_carry = pl->alloc((size_t)carry64 * 64 + 64); ok = pl->d_carry != nullptr; }
    if (!ok) {
        fail(CLH_E_HIP, "out of device memory or upload failed while building the edit-matrix plan");
        delete pl; return nullptr;
    }
    return pl;
}

extern "C" int clh_edit_matrix_plan_run(clh_edit_matrix_plan* pl, void* stream_)
{
    if (!pl) return fail(CLH_E_ARG, "clh_edit_matrix_plan_run: null argument");
    hipStream_t st;
    if (int rc = pl->begin_run(stream_, &st)) return rc;
    HIPCHK(hipMemsetAsync(pl->d_ctl, 0, sizeof(clh::EmCtl), st));
    if (pl->hpc) HIPCHK(clh::launch_hpc_compress((const uint8_t*)pl->d_raw, (const int64_t*)pl->d_seq_off, pl->nseq, (uint8_t*)pl->d_hpc, (int32_t*)pl->d_len, st));
    clh::EmParams p;
    p.seq_off = (const int64_t*)pl->d_seq_off; p.len = (const int32_t*)pl->d_len;
    p.group_off = (const int64_t*)pl->d_group_off; p.pair_base = (const int64_t*)pl->d_pair_base;
    p.ngroups = pl->ngroups; p.npairs = pl->npairs;
    p.tasks = (clh::EdTask*)pl->d_tasks; p.out = (int32_t*)pl->d_out; p.ctl = (clh::EmCtl*)pl->d_ctl; p.carry_cap64 = pl->carry_cap64;
    HIPCHK(clh::launch_edit_matrix_tasks(p, false, st));
    HIPCHK(clh::launch_edit_matrix_tasks(p, true, st));
    // the one read-back: how many pairs each class holds (and the lengths, which fetch and sizes report)
    HIPCHK(hipMemcpyAsync(&pl->ctl, pl->d_ctl, sizeof(clh::EmCtl), hipMemcpyDeviceToHost, st));
    if (pl->hpc && pl->nseq) HIPCHK(hipMemcpyAsync(pl->len.data(), pl->d_len, sizeof(int32_t) * (size_t)pl->nseq, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (pl->ctl.no_carry) {
        // such a pair was counted in its class but has no task: the class lists are not complete, so K4 does not run on them
        if (int rc = pl->end_run()) return rc;
        return fail(CLH_E_CAPACITY, "clh_edit_matrix_plan_run: " + std::to_string(pl->ctl.no_carry) + " pairs of strings above 4096 symbols found no room for their between-pass deltas (" +
                    std::to_string(pl->ctl.carry_used64 * 64) + " bytes asked for, " + std::to_string(pl->carry_cap64 * 64) + " there)");
    }
    const uint8_t* sym = (const uint8_t*)(pl->hpc ? pl->d_hpc : pl->d_raw);
    int64_t at = 0;
    for (int c = 0; c < 7; ++c) {
        HIPCHK(clh::launch_edit_distance(sym, (const clh::EdTask*)pl->d_tasks + at, (int)pl->ctl.count[c], 1 << c, pl->planes, (int32_t*)pl->d_out, (int8_t*)pl->d_carry, st));
        at += pl->ctl.count[c];
    }
    return pl->end_run();
}

extern "C" int clh_edit_matrix_plan_sizes(clh_edit_matrix_plan* pl, int64_t* npairs, int64_t* hpc_bytes)
{
    if (!pl || !npairs || !hpc_bytes) return fail(CLH_E_ARG, "clh_edit_matrix_plan_sizes: null argument");
    if (pl->hpc && !pl->ran) return fail(CLH_E_ARG, "clh_edit_matrix_plan_sizes: the compressed size is known after clh_edit_matrix_plan_run");
    *npairs = pl->npairs;
    *hpc_bytes = 0;
    for (int32_t l : pl->len) *hpc_bytes += l;
    return 0;
}

extern "C" int clh_edit_matrix_plan_fetch(clh_edit_matrix_plan* pl, int32_t* dist, int64_t dist_cap, int32_t* len, uint8_t* hpc, int64_t hpc_cap)
{
    if (!pl || !len || (!dist && pl->npairs > 0)) return fail(CLH_E_ARG, "clh_edit_matrix_plan_fetch: null argument");
    if (!pl->ran) return fail(CLH_E_ARG, "clh_edit_matrix_plan_fetch before clh_edit_matrix_plan_run");
    if (pl->ctl.no_carry) return fail(CLH_E_CAPACITY, "clh_edit_matrix_plan_fetch: the run left " + std::to_string(pl->ctl.no_carry) + " pairs without a distance");
    if (dist_cap < pl->npairs) return fail(CLH_E_CAPACITY, "clh_edit_matrix_plan_fetch: dist_cap too small");
    HIPCHK(hipSetDevice(pl->ctx->device));
    HIPCHK(hipStreamSynchronize(pl->last_stream));
    if (pl->npairs) HIPCHK(hipMemcpy(dist, pl->d_out, sizeof(int32_t) * (size_t)pl->npairs, hipMemcpyDeviceToHost));
    int64_t bytes = 0;
    for (int s = 0; s < pl->nseq; ++s) { len[s] = pl->len[(size_t)s]; bytes += len[s]; }
    if (hpc) {
        if (hpc_cap < bytes) return fail(CLH_E_CAPACITY, "clh_edit_matrix_plan_fetch: hpc_cap too small");
        std::vector<uint8_t> sym((size_t)pl->total + 1);
        if (pl->total) HIPCHK(hipMemcpy(sym.data(), pl->hpc ? pl->d_hpc : pl->d_raw, (size_t)pl->total, hipMemcpyDeviceToHost));
        int64_t w = 0;
        for (int s = 0; s < pl->nseq; ++s) {
            const uint8_t* from = sym.data() + pl->seq_off[(size_t)s];
            for (int32_t i = 0; i < len[s]; ++i) hpc[w++] = pl->letter[from[i]];
        }
    }
    return 0;
}

extern "C" int clh_edit_matrix_plan_timing(clh_edit_matrix_plan* pl, float* ms)
{
    if (!pl || !ms || !pl->ran) return fail(CLH_E_ARG, "clh_edit_matrix_plan_timing: no run to time");
    return pl->elapsed(ms);
}

extern "C" int clh_edit_matrix_batch(clh_ctx* ctx, int32_t nseq, const uint8_t* seqs, const int64_t* seq_off, int32_t ngroups, const int64_t* group_off,
                                     int32_t flags, int32_t* dist, int64_t dist_cap, int32_t* len, uint8_t* hpc, int64_t hpc_cap)
{
    clh_edit_matrix_plan* pl = clh_edit_matrix_plan_create(ctx, nseq, seqs, seq_off, ngroups, group_off, flags);
    if (!pl) return g_code;
    int rc = clh_edit_matrix_plan_run(pl, nullptr);
    if (!rc) rc = clh_edit_matrix_plan_fetch(pl, dist, dist_cap, len, hpc, hpc_cap);
    delete pl;
    return rc;
}

// ---------------------------------------------------------------------------------------------------------------
// K4m / K4t: edlib.align -- modes NW / SHW / HW, end and start locations, CIGARs (edit_align.hip)
// ---------------------------------------------------------------------------------------------------------------
struct clh_edit_align_plan : clh_owned {
    using clh_owned::clh_owned;
    int n = 0, nk = 0, planes = 3, mode = 0, task = 0, k = -1;
    bool eq = false, starts = false;
    std::vector<int32_t> qlen, tlen, alpha, kidx;     // per pair; kidx: index among the pairs that reach the kernels, -1 trivial
    std::vector<clh::EaPair> kp;
    std::vector<clh::EaTask> tasks;                  // K4m, launch order (by lane-group class, longest text first)
    int64_t ends_total = 0, nslots = 0;
    struct Launch { int64_t a, b; int G; };
    std::vector<Launch> rev;                         // reverse-pass launches over slot ranges
    std::vector<clh::EaPath> paths;                  // K4t tasks, by chunk, then lane-group class
    std::vector<int64_t> cig_of;                     // per kernel pair: its CIGAR's first op in the device buffer, -1 none
    struct Chunk { int a, b; std::vector<Launch> cls; };
    std::vector<Chunk> chunks;
    int64_t cig_total = 0, ws_bytes = 0, carry_score = 0, carry_rev = 0, carry_path = 0;
    void *d_sym = nullptr, *d_tasks = nullptr, *d_pairs = nullptr, *d_best = nullptr, *d_cnt = nullptr, *d_ends = nullptr, *d_rev_out = nullptr,
         *d_slot_pair = nullptr, *d_rev_tasks = nullptr, *d_paths = nullptr, *d_path_tasks = nullptr, *d_ws = nullptr, *d_cig = nullptr,
         *d_cig_len = nullptr, *d_carry_score = nullptr, *d_carry_rev = nullptr, *d_carry_path = nullptr, *d_eq_off = nullptr,
         *d_eq_list = nullptr, *d_eqm = nullptr;
};

static int ea_group(int m) { int B = (m + 63) >> 6, G = 1; while (G < B && G < 64) G <<= 1; return G; }
static int64_t ea_pad(int64_t n) { return ((n + 63) & ~(int64_t)63) + 64; }   // one between-pass delta buffer (as K4)

extern "C" void clh_edit_align_plan_destroy(clh_edit_align_plan* pl) { delete pl; }

extern "C" clh_edit_align_plan* clh_edit_align_plan_create(clh_ctx* ctx, int32_t n, const uint8_t* q, const int64_t* q_off, const uint8_t* t,
                                                           const int64_t* t_off, const clh_edit_align_opts* opts)
{
    if (!ctx || n < 0 || !q_off || !t_off || !opts || (n > 0 && (!q || !t))) { fail(CLH_E_ARG, "clh_edit_align_plan_create: null argument"); return nullptr; }
    if (opts->mode < CLH_EA_NW || opts->mode > CLH_EA_HW) { fail(CLH_E_ARG, "clh_edit_align_plan_create: mode must be NW, SHW or HW"); return nullptr; }
    if (opts->task < CLH_EA_DISTANCE || opts->task > CLH_EA_PATH) { fail(CLH_E_ARG, "clh_edit_align_plan_create: task must be distance, locations or path"); return nullptr; }
    if (opts->n_eq < 0 || (opts->n_eq > 0 && !opts->eq) || opts->workspace_bytes < 0) { fail(CLH_E_ARG, "clh_edit_align_plan_create: bad equalities or workspace"); return nullptr; }
    if (hipSetDevice(ctx->device) != hipSuccess) { fail(CLH_E_HIP, "hipSetDevice failed"); return nullptr; }
    const int64_t tq = n ? q_off[n] - q_off[0] : 0, tt = n ? t_off[n] - t_off[0] : 0;
    if (tq < 0 || tt < 0) { fail(CLH_E_ARG, "clh_edit_align_plan_create: offsets must ascend"); return nullptr; }
    for (int k = 0; k < n; ++k)
        if (q_off[k + 1] < q_off[k] || t_off[k + 1] < t_off[k] || q_off[k + 1] - q_off[k] > INT32_MAX / 4 || t_off[k + 1] - t_off[k] > INT32_MAX / 4) {
            fail(CLH_E_ARG, "clh_edit_align_plan_create: offsets must ascend, strings below 2^29 bytes"); return nullptr;
        }
    clh_edit_align_plan* pl = new clh_edit_align_plan(ctx);
    pl->n = n; pl->mode = opts->mode; pl->task = opts->task; pl->k = opts->k;
    pl->starts = opts->mode == CLH_EA_HW && opts->task >= CLH_EA_LOCATIONS;
    const int64_t ws_limit = opts->workspace_bytes > 0 ? opts->workspace_bytes : ((int64_t)1 << 30);
    // the batch's alphabet -> dense codes (bit planes: 3 for <= 8 letters, else 8), as K4
    int code[256];
    for (int& c : code) c = -1;
    int nsym = 0;
    auto learn = [&](const uint8_t* p, int64_t len) { for (int64_t i = 0; i < len; ++i) if (code[p[i]] < 0) code[p[i]] = nsym++; };
    if (n) { learn(q + q_off[0], tq); learn(t + t_off[0], tt); }
    pl->planes = nsym <= 8 ? 3 : 8;
    // additionalEqualities over the codes: partner lists (score pass) and a bit matrix (traceback); absent letters drop out
    std::vector<std::vector<uint8_t>> part(256);
    std::vector<uint32_t> eqm(256 * 8, 0);
    for (int e = 0; e < opts->n_eq; ++e) {
        const int a = code[opts->eq[2 * e]], b = code[opts->eq[2 * e + 1]];
        if (a < 0 || b < 0 || a == b || ((eqm[a * 8 + (b >> 5)] >> (b & 31)) & 1u)) continue;
        eqm[a * 8 + (b >> 5)] |= 1u << (b & 31); eqm[b * 8 + (a >> 5)] |= 1u << (a & 31);
        part[a].push_back((uint8_t)b); part[b].push_back((uint8_t)a);
        pl->eq = true;
    }
    std::vector<int32_t> eq_off(257, 0);
    std::vector<uint8_t> eq_list;
    for (int c = 0; c < 256; ++c) { eq_list.insert(eq_list.end(), part[c].begin(), part[c].end()); eq_off[c + 1] = (int32_t)eq_list.size(); }
    eq_list.push_back(0);
    // symbols: queries, targets, then (HW with starts) the reversed strings of the pairs that reach the kernels
    pl->qlen.resize(n); pl->tlen.resize(n); pl->alpha.resize(n); pl->kidx.assign(n, -1);
    int64_t rev_bytes = 0;
    for (int k = 0; k < n; ++k) {
        const int m = (int)(q_off[k + 1] - q_off[k]), L = (int)(t_off[k + 1] - t_off[k]);
        pl->qlen[k] = m; pl->tlen[k] = L;
        uint64_t seen[4] = {0, 0, 0, 0};
        for (int i = 0; i < m; ++i) { const int c = q[q_off[k] + i]; seen[c >> 6] |= 1ull << (c & 63); }
        for (int i = 0; i < L; ++i) { const int c = t[t_off[k] + i]; seen[c >> 6] |= 1ull << (c & 63); }
        pl->alpha[k] = __builtin_popcountll(seen[0]) + __builtin_popcountll(seen[1]) + __builtin_popcountll(seen[2]) + __builtin_popcountll(seen[3]);
        if (m > 0 && L > 0) { pl->kidx[k] = pl->nk++; if (pl->starts) rev_bytes += m + L; }
    }
    std::vector<uint8_t> sym((size_t)(tq + tt + rev_bytes) + 32, 0);
    for (int64_t i = 0; i < tq; ++i) sym[(size_t)i] = (uint8_t)code[q[q_off[0] + i]];
    for (int64_t i = 0; i < tt; ++i) sym[(size_t)(tq + i)] = (uint8_t)code[t[t_off[0] + i]];
    int64_t rpos = tq + tt;
    pl->kp.resize(pl->nk);
    for (int k = 0; k < n; ++k) {
        if (pl->kidx[k] < 0) continue;
        clh::EaPair& p = pl->kp[pl->kidx[k]];
        p.m = pl->qlen[k]; p.n = pl->tlen[k];
        p.q_off = q_off[k] - q_off[0]; p.t_off = tq + (t_off[k] - t_off[0]);
        p.rq_off = p.rt_off = 0;
        if (pl->starts) {
            p.rq_off = rpos; for (int i = 0; i < p.m; ++i) sym[(size_t)(rpos + i)] = sym[(size_t)(p.q_off + p.m - 1 - i)]; rpos += p.m;
            p.rt_off = rpos; for (int i = 0; i < p.n; ++i) sym[(size_t)(rpos + i)] = sym[(size_t)(p.t_off + p.n - 1 - i)]; rpos += p.n;
        }
        p.locbase = pl->ends_total; pl->ends_total += (int64_t)p.n + 1;
        p.slot_base = 0; p.rev_carry_stride = 0; p.rev_chunk = 1; p.rev_s0 = 0;
    }
    // K4m tasks (the carry buffers of patterns above 4096 symbols as K4's)
    for (int j = 0; j < pl->nk; ++j) {
        const clh::EaPair& p = pl->kp[j];
        clh::EaTask tk;
        tk.pat_off = p.q_off; tk.txt_off = p.t_off; tk.out_off = p.locbase; tk.carry_off = -1;
        tk.pat_len = p.m; tk.txt_len = p.n; tk.pair = j; tk.hin0 = pl->mode == CLH_EA_HW ? 0 : 1;
        if (p.m > 4096) { tk.carry_off = pl->carry_score; pl->carry_score += 2 * ea_pad(p.n); }
        pl->tasks.push_back(tk);
    }
    std::stable_sort(pl->tasks.begin(), pl->tasks.end(), [&](const clh::EaTask& x, const clh::EaTask& y) {
        const int gx = ea_group(x.pat_len), gy = ea_group(y.pat_len);
        if (gx != gy) return gx < gy;
        return x.txt_len > y.txt_len;
    });
    // reverse-pass slots: n + 1 per pair (one per possible optimal column), in K4m's order; patterns above 4096 symbols
    // take their carry buffers per slot, at most kRevCarry bytes per launch
    std::vector<int32_t> slot_pair;
    if (pl->starts) {
        const int64_t kRevCarry = (int64_t)256 << 20;
        for (size_t i = 0; i < pl->tasks.size();) {
            const int G = ea_group(pl->tasks[i].pat_len);
            size_t j = i;
            int64_t s0 = pl->nslots, pmax = 0;
            for (; j < pl->tasks.size() && ea_group(pl->tasks[j].pat_len) == G; ++j) {
                clh::EaPair& p = pl->kp[pl->tasks[j].pair];
                p.slot_base = pl->nslots; pl->nslots += (int64_t)p.n + 1;
                for (int64_t s = 0; s <= p.n; ++s) slot_pair.push_back(pl->tasks[j].pair);
                if (p.m > 4096) pmax = std::max<int64_t>(pmax, std::min<int64_t>(p.n, 2 * (int64_t)p.m + 1));
            }
            const int64_t s1 = pl->nslots;
            int64_t chunk = s1 - s0;
            if (pmax > 0) {
                const int64_t cs = 2 * ea_pad(pmax);
                chunk = std::max<int64_t>(1, kRevCarry / cs);
                for (size_t x = i; x < j; ++x) {
                    clh::EaPair& p = pl->kp[pl->tasks[x].pair];
                    p.rev_chunk = chunk; p.rev_s0 = s0; p.rev_carry_stride = p.m > 4096 ? cs : 0;
                }
                pl->carry_rev = std::max(pl->carry_rev, std::min(chunk, s1 - s0) * cs);
            }
            for (int64_t a = s0; a < s1; a += chunk) pl->rev.push_back({a, std::min(a + chunk, s1), G});
            i = j;
        }
    }
    // K4t: per pair Pv, Mv, bottom score per block and column of target[start..end]; end - start + 1 <= n, and <= 2m
    // outside NW (an optimal alignment of cost <= m spans at most 2m columns).  Chunks of the batch within ws_limit.
    pl->cig_of.assign((size_t)pl->nk, -1);
    if (pl->task == CLH_EA_PATH) {
        std::vector<clh::EaPath> all;
        std::vector<int64_t> wsb;
        for (int k = 0; k < n; ++k) {
            const int j = pl->kidx[k];
            if (j < 0) continue;
            const clh::EaPair& p = pl->kp[j];
            const int64_t lmax = pl->mode == CLH_EA_NW ? p.n : std::min<int64_t>(p.n, 2 * (int64_t)p.m);
            const int64_t B = (p.m + 63) >> 6;
            const int64_t b = (20 * B * lmax + 255) & ~(int64_t)255;
            if (b > ws_limit) {
                fail(CLH_E_CAPACITY, "clh_edit_align_plan_create: the path of pair " + std::to_string(k) + " needs " + std::to_string(b) +
                                     " bytes of workspace, above the limit of " + std::to_string(ws_limit));
                delete pl; return nullptr;
            }
            clh::EaPath ph;
            ph.pair = j; ph.lmax = (int32_t)lmax; ph.cig_cap = (int32_t)(p.m + lmax + 1); ph.pad = 0;
            ph.cig_off = pl->cig_total; pl->cig_total += ph.cig_cap;
            pl->cig_of[(size_t)j] = ph.cig_off;
            ph.ws_off = 0; ph.carry_off = -1;
            all.push_back(ph); wsb.push_back(b);
        }
        for (size_t i = 0; i < all.size();) {
            size_t j = i;
            int64_t used = 0, cused = 0;
            while (j < all.size() && (j == i || used + wsb[j] <= ws_limit)) { used += wsb[j]; ++j; }
            std::vector<clh::EaPath> part_(all.begin() + i, all.begin() + j);
            std::stable_sort(part_.begin(), part_.end(), [&](const clh::EaPath& x, const clh::EaPath& y) {
                const int gx = ea_group(pl->kp[x.pair].m), gy = ea_group(pl->kp[y.pair].m);
                if (gx != gy) return gx < gy;
                return x.lmax > y.lmax;
            });
            clh_edit_align_plan::Chunk ch;
            ch.a = (int)pl->paths.size();
            used = 0;
            for (clh::EaPath ph : part_) {
                const clh::EaPair& p = pl->kp[ph.pair];
                ph.ws_off = used; used += (20 * (((int64_t)p.m + 63) >> 6) * ph.lmax + 255) & ~(int64_t)255;
                if (p.m > 4096) { ph.carry_off = cused; cused += 2 * ea_pad(ph.lmax); }
                const int G = ea_group(p.m);
                const int64_t x = (int64_t)pl->paths.size();
                if (ch.cls.empty() || ch.cls.back().G != G) ch.cls.push_back({x, x + 1, G}); else ch.cls.back().b = x + 1;
                pl->paths.push_back(ph);
            }
            ch.b = (int)pl->paths.size();
            pl->chunks.push_back(ch);
            pl->ws_bytes = std::max(pl->ws_bytes, used);
            pl->carry_path = std::max(pl->carry_path, cused);
            i = j;
        }
    }
    const size_t nk = (size_t)std::max(pl->nk, 1);
    // a block for every buffer, even an empty one (the kernels take the pointers as they are)
    auto put = [&](const void* host, size_t bytes, size_t min_bytes) { return bytes ? pl->upload(host, bytes) : pl->alloc(min_bytes); };
    pl->d_sym = pl->upload(sym.data(), sym.size());
    pl->d_tasks = put(pl->tasks.data(), sizeof(clh::EaTask) * pl->tasks.size(), sizeof(clh::EaTask));
    pl->d_pairs = put(pl->kp.data(), sizeof(clh::EaPair) * pl->kp.size(), sizeof(clh::EaPair));
    pl->d_best = pl->alloc(4 * nk); pl->d_cnt = pl->alloc(4 * nk); pl->d_cig_len = pl->alloc(4 * nk);
    pl->d_ends = pl->alloc(4 * (size_t)std::max<int64_t>(pl->ends_total, 1));
    pl->d_rev_out = pl->alloc(4 * (size_t)(pl->starts ? std::max<int64_t>(pl->ends_total, 1) : 1));
    pl->d_slot_pair = put(slot_pair.data(), 4 * slot_pair.size(), 4);
    pl->d_rev_tasks = pl->alloc(sizeof(clh::EaTask) * (size_t)std::max<int64_t>(pl->nslots, 1));
    pl->d_paths = put(pl->paths.data(), sizeof(clh::EaPath) * pl->paths.size(), sizeof(clh::EaPath));
    pl->d_path_tasks = pl->alloc(sizeof(clh::EaTask) * std::max<size_t>(pl->paths.size(), 1));
    pl->d_ws = pl->alloc((size_t)std::max<int64_t>(pl->ws_bytes, 256));
    pl->d_cig = pl->alloc(4 * (size_t)std::max<int64_t>(pl->cig_total, 1));
    pl->d_carry_score = pl->alloc((size_t)pl->carry_score + 64);
    pl->d_carry_rev = pl->alloc((size_t)pl->carry_rev + 64);
    pl->d_carry_path = pl->alloc((size_t)pl->carry_path + 64);
    pl->d_eq_off = pl->upload(eq_off.data(), 4 * eq_off.size());
    pl->d_eq_list = pl->upload(eq_list.data(), eq_list.size());
    pl->d_eqm = pl->upload(eqm.data(), 4 * eqm.size());
    if (!pl->d_sym || !pl->d_tasks || !pl->d_pairs || !pl->d_best || !pl->d_cnt || !pl->d_cig_len || !pl->d_ends || !pl->d_rev_out || !pl->d_slot_pair ||
        !pl->d_rev_tasks || !pl->d_paths || !pl->d_path_tasks || !pl->d_ws || !pl->d_cig || !pl->d_carry_score || !pl->d_carry_rev || !pl->d_carry_path ||
        !pl->d_eq_off || !pl->d_eq_list || !pl->d_eqm) {
        fail(CLH_E_HIP, "out of device memory or upload failed while building the edit-align plan");
        delete pl; return nullptr;
    }
    return pl;
}

static clh::EaParams ea_params(const clh_edit_align_plan* pl)
{
    clh::EaParams p;
    p.sym = (const uint8_t*)pl->d_sym;
    p.best = (int32_t*)pl->d_best; p.cnt = (int32_t*)pl->d_cnt; p.ends = (int32_t*)pl->d_ends; p.ends_cap = pl->ends_total;
    p.rev_out = (int32_t*)pl->d_rev_out; p.rev_cap = pl->starts ? pl->ends_total : 0;
    p.ws = (uint8_t*)pl->d_ws; p.ws_cap = pl->ws_bytes;
    p.carry = nullptr; p.carry_cap = 0;
    p.eq_off = (const int32_t*)pl->d_eq_off; p.eq_list = (const uint8_t*)pl->d_eq_list; p.eqm = (const uint32_t*)pl->d_eqm;
    p.mode = pl->mode; p.k = pl->k;
    return p;
}

extern "C" int clh_edit_align_plan_run(clh_edit_align_plan* pl, void* stream_)
{
    if (!pl) return fail(CLH_E_ARG, "clh_edit_align_plan_run: null argument");
    hipStream_t st;
    if (int rc = pl->begin_run(stream_, &st)) return rc;
    const size_t nk = (size_t)std::max(pl->nk, 1);
    HIPCHK(hipMemsetAsync(pl->d_cnt, 0xff, 4 * nk, st));       // -1: no result (a kernel that left a pair out is caught by fetch)
    HIPCHK(hipMemsetAsync(pl->d_cig_len, 0xff, 4 * nk, st));
    if (pl->starts) HIPCHK(hipMemsetAsync(pl->d_rev_out, 0xff, 4 * (size_t)std::max<int64_t>(pl->ends_total, 1), st));
    clh::EaParams p = ea_params(pl);
    const int nt = (int)pl->tasks.size();
    p.carry = (int8_t*)pl->d_carry_score; p.carry_cap = pl->carry_score;
    for (int i = 0; i < nt;) {
        const int G = ea_group(pl->tasks[(size_t)i].pat_len);
        int j = i;
        while (j < nt && ea_group(pl->tasks[(size_t)j].pat_len) == G) ++j;
        HIPCHK(clh::launch_edit_align(p, clh::EA_SCORE, (const clh::EaTask*)pl->d_tasks + i, j - i, G, pl->planes, pl->eq, st));
        i = j;
    }
    if (pl->starts && pl->nslots) {
        clh::EaTask* rt = (clh::EaTask*)pl->d_rev_tasks;
        HIPCHK(clh::launch_edit_align_build_rev(p, (const clh::EaPair*)pl->d_pairs, (const int32_t*)pl->d_slot_pair, pl->nslots, rt, st));
        p.carry = (int8_t*)pl->d_carry_rev; p.carry_cap = pl->carry_rev;
        for (const auto& l : pl->rev)
            HIPCHK(clh::launch_edit_align(p, clh::EA_REVERSE, rt + l.a, (int)(l.b - l.a), l.G, pl->planes, pl->eq, st));
    }
    p.carry = (int8_t*)pl->d_carry_path; p.carry_cap = pl->carry_path;
    for (const auto& ch : pl->chunks) {
        const clh::EaPath* ph = (const clh::EaPath*)pl->d_paths + ch.a;
        clh::EaTask* pt = (clh::EaTask*)pl->d_path_tasks + ch.a;
        HIPCHK(clh::launch_edit_align_build_path(p, (const clh::EaPair*)pl->d_pairs, ph, ch.b - ch.a, pt, st));
        for (const auto& l : ch.cls)
            HIPCHK(clh::launch_edit_align(p, clh::EA_STORE, (const clh::EaTask*)pl->d_path_tasks + l.a, (int)(l.b - l.a), l.G, pl->planes, pl->eq, st));
        HIPCHK(clh::launch_edit_align_traceback(p, ph, pt, ch.b - ch.a, (uint32_t*)pl->d_cig, (int32_t*)pl->d_cig_len, st));
    }
    return pl->end_run();
}

// capacities: a pair has at most n + 1 optimal columns; its CIGAR at most m + n ops
static void ea_caps(const clh_edit_align_plan* pl, int64_t* lc, int64_t* cc)
{
    *lc = 0; *cc = 0;
    for (int k = 0; k < pl->n; ++k) { *lc += (int64_t)pl->tlen[k] + 1; *cc += (int64_t)pl->qlen[k] + pl->tlen[k] + 1; }
}

extern "C" int clh_edit_align_plan_caps(clh_edit_align_plan* pl, int64_t* locs_cap, int64_t* cigar_cap)
{
    if (!pl || !locs_cap || !cigar_cap) return fail(CLH_E_ARG, "clh_edit_align_plan_caps: null argument");
    ea_caps(pl, locs_cap, cigar_cap);
    return 0;
}

extern "C" int clh_edit_align_plan_fetch(clh_edit_align_plan* pl, clh_edit_align_row* rows, int32_t* locs, int64_t locs_cap, int64_t* locs_used,
                                         uint32_t* cigar, int64_t cigar_cap, int64_t* cigar_used)
{
    if (!pl || !rows || !locs_used || !cigar_used || (locs_cap > 0 && !locs) || (cigar_cap > 0 && !cigar))
        return fail(CLH_E_ARG, "clh_edit_align_plan_fetch: null argument");
    if (!pl->ran) return fail(CLH_E_ARG, "clh_edit_align_plan_fetch before clh_edit_align_plan_run");
    HIPCHK(hipSetDevice(pl->ctx->device));
    HIPCHK(hipStreamSynchronize(pl->last_stream));
    const size_t nk = (size_t)std::max(pl->nk, 1);
    std::vector<int32_t> best(nk), cnt(nk), cl(nk), ends((size_t)std::max<int64_t>(pl->ends_total, 1)), rev(pl->starts ? ends.size() : 0);
    std::vector<uint32_t> cig((size_t)std::max<int64_t>(pl->cig_total, 1));
    if (pl->nk) {
        HIPCHK(hipMemcpy(best.data(), pl->d_best, 4 * nk, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(cnt.data(), pl->d_cnt, 4 * nk, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(cl.data(), pl->d_cig_len, 4 * nk, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(ends.data(), pl->d_ends, 4 * ends.size(), hipMemcpyDeviceToHost));
        if (pl->starts) HIPCHK(hipMemcpy(rev.data(), pl->d_rev_out, 4 * rev.size(), hipMemcpyDeviceToHost));
        if (pl->cig_total) HIPCHK(hipMemcpy(cig.data(), pl->d_cig, 4 * (size_t)pl->cig_total, hipMemcpyDeviceToHost));
    }
    const bool want_start = pl->task >= CLH_EA_LOCATIONS, want_path = pl->task == CLH_EA_PATH;
    int64_t lu = 0, cu = 0;
    std::vector<int32_t> le;     // this pair's (start, end)
    std::vector<uint32_t> ops;
    for (int k = 0; k < pl->n; ++k) {
        const int m = pl->qlen[k], L = pl->tlen[k], j = pl->kidx[k];
        int d;
        le.clear(); ops.clear();
        if (j < 0) {
            // an empty side: the dynamic programme's own answer (column -1 = before the first target letter)
            if (L == 0) { d = m; le = {0, -1}; if (m) ops.push_back(((uint32_t)m << 4) | 1u); }
            else if (pl->mode == CLH_EA_NW) { d = L; le = {0, L - 1}; ops.push_back(((uint32_t)L << 4) | 2u); }
            else if (pl->mode == CLH_EA_SHW) { d = 1; le = {0, 0}; ops.push_back((1u << 4) | 2u); }
            else { d = 0; for (int e = -1; e < L; ++e) { le.push_back(e + 1); le.push_back(e); } }
        } else {
            d = best[(size_t)j];
            const int c = cnt[(size_t)j];
            const int64_t base = pl->kp[(size_t)j].locbase;
            if (c < 1 || c > L + 1) return fail(CLH_E_HIP, "edit_align: the score pass left pair " + std::to_string(k) + " without a result");
            const bool above = pl->k >= 0 && d > pl->k;
            for (int i = 0; i < c && !above; ++i) {
                const int e = ends[(size_t)(base + i)];
                int s = 0;
                if (pl->starts && e >= 0) {
                    const int p = rev[(size_t)(base + i)];
                    if (p < 0) return fail(CLH_E_HIP, "edit_align: the reverse pass left pair " + std::to_string(k) + " without a start");
                    s = e - p;
                }
                le.push_back(s); le.push_back(e);
            }
            if (want_path && !above) {
                const int n_ops = cl[(size_t)j];
                if (n_ops < 0) return fail(CLH_E_HIP, "edit_align: the traceback failed for pair " + std::to_string(k));
                const int64_t co = pl->cig_of[(size_t)j];
                if (co < 0) return fail(CLH_E_HIP, "edit_align: no path task for pair " + std::to_string(k));
                ops.assign(cig.begin() + co, cig.begin() + co + n_ops);
            }
        }
        clh_edit_align_row& r = rows[k];
        const bool above = pl->k >= 0 && d > pl->k;
        r.distance = above ? -1 : d;
        r.status = above ? CLH_EA_ST_ABOVE_K : 0;
        r.alphabet_len = pl->alpha[(size_t)k];
        r.reserved = 0;
        if (above) { le.clear(); ops.clear(); }
        r.nlocs = (int32_t)(le.size() / 2);
        r.loc_off = lu;
        if (lu + r.nlocs > locs_cap) return fail(CLH_E_CAPACITY, "clh_edit_align_plan_fetch: locs_cap too small");
        for (size_t i = 0; i < le.size(); i += 2) { locs[2 * lu] = want_start ? le[i] : -1; locs[2 * lu + 1] = le[i + 1]; ++lu; }
        r.cigar_off = want_path && !above ? cu : -1;
        r.cigar_len = want_path && !above ? (int32_t)ops.size() : 0;
        if (want_path && !above) {
            if (cu + (int64_t)ops.size() > cigar_cap) return fail(CLH_E_CAPACITY, "clh_edit_align_plan_fetch: cigar_cap too small");
            for (uint32_t o : ops) cigar[cu++] = o;
        }
    }
    *locs_used = lu; *cigar_used = cu;
    return 0;
}

extern "C" int clh_edit_align_plan_timing(clh_edit_align_plan* pl, float* ms)
{
    if (!pl || !ms || !pl->ran) return fail(CLH_E_ARG, "clh_edit_align_plan_timing: no run to time");
    return pl->elapsed(ms);
}

extern "C" int clh_edit_align_batch(clh_ctx* ctx, int32_t n, const uint8_t* q, const int64_t* q_off, const uint8_t* t, const int64_t* t_off,
                                    const clh_edit_align_opts* opts, clh_edit_align_row* rows, int32_t* locs, int64_t locs_cap, int64_t* locs_used,
                                    uint32_t* cigar, int64_t cigar_cap, int64_t* cigar_used)
{
    if (!rows || !locs_used || !cigar_used) return fail(CLH_E_ARG, "clh_edit_align_batch: null argument");
    clh_edit_align_plan* pl = clh_edit_align_plan_create(ctx, n, q, q_off, t, t_off, opts);
    if (!pl) return g_code;
    int rc = clh_edit_align_plan_run(pl, nullptr);
    if (!rc) rc = clh_edit_align_plan_fetch(pl, rows, locs, locs_cap, locs_used, cigar, cigar_cap, cigar_used);
    delete pl;
    return rc;
}

// ---------------------------------------------------------------------------------------------------------------
// K4s: probes of at most 64 letters against whole texts, HW with locations, one wave per cell (edit_search.hip)
// ---------------------------------------------------------------------------------------------------------------
struct clh_edit_search_plan : clh_owned {
    using clh_owned::clh_owned;
    int ntext = 0, nprobe = 0, k = -1, n_eq = 0;
    int64_t ncell = 0, total_chunks = 0, npart = 0;
    std::vector<int32_t> plen, tlen, list[2], split;   // list[0]: probes of 1..32 letters, list[1]: of 33..64
    void *d_text = nullptr, *d_text_off = nullptr, *d_probe = nullptr, *d_probe_off = nullptr, *d_list[2] = {nullptr, nullptr}, *d_chunk_base = nullptr,
         *d_split = nullptr, *d_eq = nullptr, *d_rows = nullptr, *d_part = nullptr;
};

extern "C" void clh_edit_search_plan_destroy(clh_edit_search_plan* pl) { delete pl; }

extern "C" clh_edit_search_plan* clh_edit_search_plan_create(clh_ctx* ctx, int32_t ntext, const uint8_t* texts, const int64_t* text_off, int32_t nprobe,
                                                             const uint8_t* probes, const int64_t* probe_off, const clh_edit_search_opts* opts)
{
    const char* me = "clh_edit_search_plan_create: ";
    if (!ctx || ntext < 0 || nprobe < 0 || !text_off || !probe_off || !opts || opts->n_eq < 0 || (opts->n_eq > 0 && !opts->eq)) {
        fail(CLH_E_ARG, std::string(me) + "bad argument"); return nullptr;
    }
    for (int t = 0; t < ntext; ++t) {
        const int64_t l = text_off[t + 1] - text_off[t];
        if (l < 0) { fail(CLH_E_ARG, std::string(me) + "offsets must ascend"); return nullptr; }
        if (l > ((int64_t)1 << 30)) { fail(CLH_E_ARG, std::string(me) + "a text of more than 2^30 bytes"); return nullptr; }
    }
    for (int q = 0; q < nprobe; ++q) {
        const int64_t l = probe_off[q + 1] - probe_off[q];
        if (l < 0) { fail(CLH_E_ARG, std::string(me) + "offsets must ascend"); return nullptr; }
        if (l > 64) { fail(CLH_E_ARG, std::string(me) + "a probe of more than 64 letters (clh_edit_align_batch takes those)"); return nullptr; }
    }
    const int64_t tt = text_off[ntext] - text_off[0], tp = probe_off[nprobe] - probe_off[0];
    if ((tt > 0 && !texts) || (tp > 0 && !probes)) { fail(CLH_E_ARG, std::string(me) + "null argument"); return nullptr; }
    if (hipSetDevice(ctx->device) != hipSuccess) { fail(CLH_E_HIP, "hipSetDevice failed"); return nullptr; }
    clh_edit_search_plan* pl = new clh_edit_search_plan(ctx);
    pl->ntext = ntext; pl->nprobe = nprobe; pl->k = opts->k; pl->n_eq = opts->n_eq;
    pl->ncell = (int64_t)ntext * nprobe;
    std::vector<int64_t> toff((size_t)ntext + 1), poff((size_t)nprobe + 1), chunk_base((size_t)ntext + 1, 0);
    for (int t = 0; t <= ntext; ++t) toff[(size_t)t] = text_off[t] - text_off[0];
    for (int q = 0; q <= nprobe; ++q) poff[(size_t)q] = probe_off[q] - probe_off[0];
    pl->tlen.resize((size_t)ntext); pl->plen.resize((size_t)nprobe);
    for (int t = 0; t < ntext; ++t) {
        const int64_t l = toff[(size_t)t + 1] - toff[(size_t)t];
        const int64_t nch = std::max<int64_t>(1, (l + clh::kEsChunk - 1) / clh::kEsChunk);   // an empty text keeps one chunk: its cells are the kernel's too
        pl->tlen[(size_t)t] = (int32_t)l;
        chunk_base[(size_t)t + 1] = chunk_base[(size_t)t] + nch;
        if (nch > 1) pl->split.push_back(t);
    }
    pl->total_chunks = chunk_base[(size_t)ntext];
    for (int q = 0; q < nprobe; ++q) {
        const int l = (int)(poff[(size_t)q + 1] - poff[(size_t)q]);
        pl->plen[(size_t)q] = l;
        if (l > 0) pl->list[l > 32].push_back(q);           // an empty probe is answered by fetch
    }
    pl->npart = pl->split.empty() ? 0 : (int64_t)nprobe * pl->total_chunks;
    pl->d_text = pl->upload(texts ? texts + text_off[0] : nullptr, (size_t)tt);
    pl->d_probe = pl->upload(probes ? probes + probe_off[0] : nullptr, (size_t)tp);
    pl->d_text_off = pl->upload(toff.data(), sizeof(int64_t) * toff.size());
    pl->d_probe_off = pl->upload(poff.data(), sizeof(int64_t) * poff.size());
    pl->d_chunk_base = pl->upload(chunk_base.data(), sizeof(int64_t) * chunk_base.size());
    pl->d_split = pl->upload(pl->split.data(), sizeof(int32_t) * pl->split.size());
    pl->d_eq = pl->upload(opts->eq, 2 * (size_t)opts->n_eq);
    for (int w = 0; w < 2; ++w) pl->d_list[w] = pl->upload(pl->list[w].data(), sizeof(int32_t) * pl->list[w].size());
    pl->d_rows = pl->alloc(sizeof(clh_edit_search_row) * (size_t)std::max<int64_t>(pl->ncell, 1));
    pl->d_part = pl->alloc(16 * (size_t)std::max<int64_t>(pl->npart, 1));
    if (!pl->d_text || !pl->d_probe || !pl->d_text_off || !pl->d_probe_off || !pl->d_chunk_base || !pl->d_split || !pl->d_eq || !pl->d_list[0] ||
        !pl->d_list[1] || !pl->d_rows || !pl->d_part) {
        fail(CLH_E_HIP, "out of device memory or upload failed while building the edit-search plan");
        delete pl; return nullptr;
    }
    return pl;
}

extern "C" int clh_edit_search_plan_run(clh_edit_search_plan* pl, void* stream_)
{
    if (!pl) return fail(CLH_E_ARG, "clh_edit_search_plan_run: null argument");
    hipStream_t st;
    if (int rc = pl->begin_run(stream_, &st)) return rc;
    // every cell and every chunk tuple starts as "unwritten": what a kernel did not store is reported by fetch, never returned
    if (pl->ncell) HIPCHK(hipMemsetAsync(pl->d_rows, 0x80, sizeof(clh_edit_search_row) * (size_t)pl->ncell, st));
    if (pl->npart) HIPCHK(hipMemsetAsync(pl->d_part, 0x80, 16 * (size_t)pl->npart, st));
    clh::EsParams p;
    p.text = (const uint8_t*)pl->d_text; p.text_off = (const int64_t*)pl->d_text_off;
    p.probe = (const uint8_t*)pl->d_probe; p.probe_off = (const int64_t*)pl->d_probe_off;
    p.chunk_base = (const int64_t*)pl->d_chunk_base;
    p.split_list = (const int32_t*)pl->d_split; p.nsplit = (int32_t)pl->split.size();
    p.eq = (const uint8_t*)pl->d_eq; p.n_eq = pl->n_eq;
    p.ntext = pl->ntext; p.nprobe = pl->nprobe; p.k = pl->k;
    p.total_chunks = pl->total_chunks;
    p.rows = (int32_t*)pl->d_rows; p.ncell = pl->ncell;
    p.part = (int32_t*)pl->d_part; p.npart = pl->npart;
    for (int w = 0; w < 2 && pl->ntext > 0; ++w) {
        p.probe_list = (const int32_t*)pl->d_list[w]; p.nlist = (int32_t)pl->list[w].size();
        HIPCHK(clh::launch_edit_search(p, w ? 64 : 32, st));
    }
    for (int w = 0; w < 2 && p.nsplit > 0; ++w) {
        p.probe_list = (const int32_t*)pl->d_list[w]; p.nlist = (int32_t)pl->list[w].size();
        HIPCHK(clh::launch_edit_search_finish(p, w ? 64 : 32, st));
    }
    return pl->end_run();
}

extern "C" int clh_edit_search_plan_fetch(clh_edit_search_plan* pl, clh_edit_search_row* rows, int64_t rows_cap)
{
    if (!pl || (!rows && pl->ncell > 0)) return fail(CLH_E_ARG, "clh_edit_search_plan_fetch: null argument");
    if (!pl->ran) return fail(CLH_E_ARG, "clh_edit_search_plan_fetch before clh_edit_search_plan_run");
    if (rows_cap < pl->ncell) return fail(CLH_E_CAPACITY, "clh_edit_search_plan_fetch: rows_cap too small");
    if (!pl->ncell) return 0;
    HIPCHK(hipSetDevice(pl->ctx->device));
    HIPCHK(hipStreamSynchronize(pl->last_stream));
    HIPCHK(hipMemcpy(rows, pl->d_rows, sizeof(clh_edit_search_row) * (size_t)pl->ncell, hipMemcpyDeviceToHost));
    // the empty probe, stated here as align states it: distance 0 at every column from -1 on, start = end + 1
    for (int q = 0; q < pl->nprobe; ++q) {
        if (pl->plen[(size_t)q]) continue;
        for (int t = 0; t < pl->ntext; ++t) {
            const int32_t n = pl->tlen[(size_t)t];
            rows[(int64_t)t * pl->nprobe + q] = clh_edit_search_row{0, 0, -1, n - 1, n + 1};
        }
    }
    int64_t unwritten = 0;
    for (int64_t c = 0; c < pl->ncell; ++c) unwritten += rows[c].distance == clh::kEsUnwritten || rows[c].nlocs == clh::kEsUnwritten;
    if (unwritten) return fail(CLH_E_HIP, "clh_edit_search_plan_fetch: the kernels left " + std::to_string(unwritten) + " cells unwritten");
    return 0;
}

extern "C" int clh_edit_search_plan_timing(clh_edit_search_plan* pl, float* ms)
{
    if (!pl || !ms || !pl->ran) return fail(CLH_E_ARG, "clh_edit_search_plan_timing: no run to time");
    return pl->elapsed(ms);
}

extern "C" int clh_edit_search_plan_info(clh_edit_search_plan* pl, int64_t* out)
{
    if (!pl || !out) return fail(CLH_E_ARG, "clh_edit_search_plan_info: null argument");
    out[0] = clh::kEsSeg; out[1] = clh::kEsRound; out[2] = clh::kEsChunk; out[3] = pl->ntext;
    out[4] = pl->total_chunks; out[5] = (int64_t)pl->split.size(); out[6] = (int64_t)pl->list[0].size(); out[7] = (int64_t)pl->list[1].size();
    return 0;
}

extern "C" int clh_edit_search_batch(clh_ctx* ctx, int32_t ntext, const uint8_t* texts, const int64_t* text_off, int32_t nprobe, const uint8_t* probes,
                                     const int64_t* probe_off, const clh_edit_search_opts* opts, clh_edit_search_row* rows, int64_t rows_cap)
{
    clh_edit_search_plan* pl = clh_edit_search_plan_create(ctx, ntext, texts, text_off, nprobe, probes, probe_off, opts);
    if (!pl) return g_code;
    int rc = clh_edit_search_plan_run(pl, nullptr);
    if (!rc) rc = clh_edit_search_plan_fetch(pl, rows, rows_cap);
    delete pl;
    return rc;
}

// ---------------------------------------------------------------------------------------------------------------
// K1g and K1gb: what the two pair plans share on the host.  A create checks and plans everything here (pairs, CIGAR room, the
// shares of the workspace) before its first device call; a run starts and fetch reads the same way for both.
// ---------------------------------------------------------------------------------------------------------------
// clh_band_opts and clh_band_row begin with the fields of clh_ends_opts and clh_ends_row: one option check and one row writer serve both
static_assert(offsetof(clh_band_opts, mode) == offsetof(clh_ends_opts, mode) && offsetof(clh_band_opts, mat) == offsetof(clh_ends_opts, mat) &&
              offsetof(clh_band_opts, n_mat) == offsetof(clh_ends_opts, n_mat) && offsetof(clh_band_opts, gap_open) == offsetof(clh_ends_opts, gap_open) &&
              offsetof(clh_band_opts, gap_extend) == offsetof(clh_ends_opts, gap_extend) && offsetof(clh_band_opts, want_cigar) == offsetof(clh_ends_opts, want_cigar) &&
              offsetof(clh_band_opts, workspace_bytes) == offsetof(clh_ends_opts, workspace_bytes) && offsetof(clh_band_opts, band) == sizeof(clh_ends_opts),
              "clh_band_opts begins with clh_ends_opts");
static_assert(offsetof(clh_band_row, score) == offsetof(clh_ends_row, score) && offsetof(clh_band_row, ref_begin) == offsetof(clh_ends_row, ref_begin) &&
              offsetof(clh_band_row, ref_end) == offsetof(clh_ends_row, ref_end) && offsetof(clh_band_row, query_begin) == offsetof(clh_ends_row, query_begin) &&
              offsetof(clh_band_row, query_end) == offsetof(clh_ends_row, query_end) && offsetof(clh_band_row, cigar_len) == offsetof(clh_ends_row, cigar_len) &&
              offsetof(clh_band_row, cigar_off) == offsetof(clh_ends_row, cigar_off) && offsetof(clh_band_row, band_lo) == sizeof(clh_ends_row),
              "clh_band_row begins with clh_ends_row");

// what a create plans on the host
struct PairsShape {
    int n = 0, mode = 0, n_mat = 0, go = 0, ge = 0;
    int pieces = 1, go2 = 0, ge2 = 0;             // two-piece gap costs (clh_gap2): a gap costs the smaller of the two pieces
    bool spliced = false;                         // intron gaps (clh_splice): K1g alone
    int io = 0;
    std::vector<int64_t> row0_intron;             // spliced, global: per pair without a query letter, what its reference costs as one intron (else -1)
    bool want_cigar = false;
    int64_t gap(int64_t k) const                  // what a gap of k >= 1 letters costs
    {
        const int64_t a = go + (k - 1) * ge;
        return pieces == 2 ? std::min<int64_t>(a, go2 + (k - 1) * (int64_t)ge2) : a;
    }
    std::vector<std::pair<int, int>> shares;      // [first, count) of each launch: the batch cut so that a share's decisions fit the workspace
    int64_t ws_bytes = 0, cig_cap = 0, max_pair_ws = 0, nempty = 0;
};
struct clh_pairs_plan : clh_owned, PairsShape {
    using clh_owned::clh_owned;
    void *d_q = nullptr, *d_r = nullptr, *d_pairs = nullptr, *d_mat = nullptr, *d_ws = nullptr, *d_rows = nullptr, *d_cig = nullptr;
    float gather_ms = -1;                         // the windows form: HIP-event time of the gather at create, and the letters it moved
    int64_t gather_letters = 0;
};

// the arguments and options both creates take, refused in the order each always refused them; `band`: K1gb's half-width, null for K1g;
// `g2`: the second piece of the gap costs, null for one piece
static int pairs_check_opts(const std::string& me, const clh_ctx* ctx, int32_t n, const int64_t* q_off, const int64_t* r_off, const clh_ends_opts* o,
                            const int32_t* band, const clh_gap2* g2 = nullptr)
{
    if (!ctx || n < 0 || !q_off || !r_off || !o || !o->mat) return fail(CLH_E_ARG, me + "bad argument");
    if (band) {
        if (o->mode == CLH_ENDS_OVERLAP) return fail(CLH_E_UNSUPPORTED, me + "overlap with a band is not built; clh_ends_plan_create takes the mode over the full matrix");
        if (o->mode < CLH_ENDS_GLOBAL || o->mode > CLH_ENDS_EXTEND) return fail(CLH_E_ARG, me + "mode must be CLH_ENDS_GLOBAL, _SEMIGLOBAL, _PREFIX or _EXTEND");
    } else if (o->mode < CLH_ENDS_GLOBAL || o->mode > CLH_ENDS_EXTEND) return fail(CLH_E_ARG, me + "mode must be CLH_ENDS_GLOBAL, _SEMIGLOBAL, _OVERLAP, _PREFIX or _EXTEND");
    if (o->n_mat < 1 || o->n_mat > 32) return fail(CLH_E_ARG, me + "n_mat must be 1..32");
    if (o->gap_open < 0 || o->gap_extend < 0 || o->workspace_bytes < 0 || (band && *band < 0))
        return fail(CLH_E_ARG, me + (band ? "gap costs, workspace_bytes and band must not be negative" : "gap costs and workspace_bytes must not be negative"));
    if (o->gap_open < o->gap_extend)
        return fail(CLH_E_UNSUPPORTED, me + "gap_open < gap_extend: E along a row is a running maximum only when opening a gap costs at least as much as extending one; not implemented");
    if (g2) {      // piece 1 for short gaps, piece 2 for long ones: 0 <= ge2 <= ge1 <= go1 <= go2
        const std::string costs = " (gap_open " + std::to_string(o->gap_open) + ", gap_extend " + std::to_string(o->gap_extend) + ", gap_open2 " +
                                  std::to_string(g2->gap_open2) + ", gap_extend2 " + std::to_string(g2->gap_extend2) + ")";
        if (g2->gap_extend2 < 0) return fail(CLH_E_UNSUPPORTED, me + "two-piece gap costs need 0 <= gap_extend2" + costs);
        if (g2->gap_extend2 > o->gap_extend) return fail(CLH_E_UNSUPPORTED, me + "two-piece gap costs need gap_extend2 <= gap_extend: the second piece is the one for long gaps" + costs);
        if (o->gap_open > g2->gap_open2) return fail(CLH_E_UNSUPPORTED, me + "two-piece gap costs need gap_open <= gap_open2: the first piece is the one for short gaps" + costs);
    }
    return 0;
}

// smax: the greatest of |s|, gap_open, gap_extend, 1, what one step moves a score by at most; *splus: max(0, greatest matrix entry)
static int64_t pairs_scan_matrix(const clh_ends_opts* o, int64_t* splus, const clh_gap2* g2 = nullptr)
{
    int64_t smax = std::max<int64_t>(std::max(o->gap_open, o->gap_extend), 1);
    if (g2) smax = std::max<int64_t>(smax, std::max(g2->gap_open2, g2->gap_extend2));
    *splus = 0;
    for (int k = 0; k < o->n_mat * o->n_mat; ++k) { smax = std::max<int64_t>(smax, std::abs((int)o->mat[k])); *splus = std::max<int64_t>(*splus, o->mat[k]); }
    return smax;
}

// Where the reference letters of a create come from: host codes (r, r_off), or windows of a resident genome that the device gathers
// into the plan's reference buffer (genome_gather.h).  Everything behind a create reads start and len alone.
struct PairsRefs {
    const int8_t* r = nullptr; const int64_t* r_off = nullptr;                                      // the strings form
    clh_genome* genome = nullptr;                                                                   // the windows form
    const int64_t* win_off = nullptr; const int32_t* win_len = nullptr; const uint8_t* win_flags = nullptr;
    std::vector<int64_t> start, len;              // reference k in the plan's buffer: its first code, its letters
    int64_t total = 0;                            // bytes of the buffer
    // what pairs_check_opts takes for r_off: the windows form has none to miss
    const int64_t* off_arg(const int64_t* q_off) const { return genome ? q_off : r_off; }
};
static PairsRefs refs_strings(const int8_t* r, const int64_t* r_off) { PairsRefs f; f.r = r; f.r_off = r_off; return f; }
static PairsRefs refs_windows(clh_genome* g, const int64_t* off, const int32_t* len, const uint8_t* flags)
{
    PairsRefs f; f.genome = g; f.win_off = off; f.win_len = len; f.win_flags = flags; return f;
}

// start, len and total, after pairs_check_opts.  Strings: the offsets as given (a descending pair is refused by the create's own
// loop).  Windows: each checked against the genome, and started on a 16-byte boundary so that the gather stores whole words.
static int pairs_ref_spans(const std::string& me, int32_t n, int n_mat, PairsRefs* f)
{
    f->start.resize((size_t)n); f->len.resize((size_t)n);
    if (!f->genome) {
        for (int k = 0; k < n; ++k) { f->start[(size_t)k] = f->r_off[k] - f->r_off[0]; f->len[(size_t)k] = f->r_off[k + 1] - f->r_off[k]; }
        f->total = n ? f->r_off[n] - f->r_off[0] : 0;
        return 0;
    }
    if (n > 0 && (!f->win_off || !f->win_len || !f->win_flags)) return fail(CLH_E_ARG, me + "null argument");
    if (n_mat != 5)
        return fail(CLH_E_UNSUPPORTED, me + "windows of the resident genome are DNA codes: the matrix must be 5 x 5, n_mat is " + std::to_string(n_mat) +
                                            "; substitution matrices over other alphabets take their references as strings");
    for (int k = 0; k < n; ++k) {
        const int64_t off = f->win_off[k], len = f->win_len[k];
        if (len < 0 || off < 0 || off + len > f->genome->len)
            return fail(CLH_E_ARG, me + "pair " + std::to_string(k) + ": the window [" + std::to_string(off) + ", " + std::to_string(off) + " + " + std::to_string(len) +
                                       ") lies outside the genome of " + std::to_string(f->genome->len) + " bases");
        if (f->win_flags[k] > 3)
            return fail(CLH_E_ARG, me + "pair " + std::to_string(k) + ": window flags must be 0..3 (bit 0 reversed, bit 1 complemented), got " + std::to_string((int)f->win_flags[k]));
        f->start[(size_t)k] = f->total; f->len[(size_t)k] = len;
        f->total += (len + clh::kGatherWord - 1) & ~(int64_t)(clh::kGatherWord - 1);
    }
    return 0;
}

// r_off null: the queries alone (the windows form, whose reference codes the gather makes)
static int pairs_check_codes(const std::string& me, int32_t n, const int8_t* q, const int64_t* q_off, const int8_t* r, const int64_t* r_off, int n_mat)
{
    for (int k = 0; k < n; ++k) {
        for (int side = 0; side < (r_off ? 2 : 1); ++side) {
            const int8_t* s = side ? r : q;
            const int64_t* off = side ? r_off : q_off;
            for (int64_t x = off[k]; x < off[k + 1]; ++x)
                if (s[x] < 0 || s[x] >= n_mat)
                    return fail(CLH_E_ARG, me + "pair " + std::to_string(k) + ": code " + std::to_string((int)s[x]) + " at letter " + std::to_string(x - off[k]) + " of the " +
                                               (side ? "reference" : "query") + " is outside the matrix (edge " + std::to_string(n_mat) + ")");
        }
    }
    return 0;
}

// Fills the fields EnPair and BdPair name alike and cuts the batch into shares.  own(k, pair, kernel) fills the pair's other fields
// and returns the bytes its stored decisions need (read only where CIGARs are wanted and the kernels take the pair); cells(pair)
// words them for the refusal of a pair that is above the workspace alone.
template <typename Pair, typename Own, typename Cells>
static int pairs_cut_shares(const std::string& me, const clh_ends_opts* o, int32_t n, const int64_t* q_off, const PairsRefs& refs, PairsShape* sh,
                            std::vector<Pair>* pairs, Own own, Cells cells)
{
    sh->n = n; sh->mode = o->mode; sh->n_mat = o->n_mat; sh->go = o->gap_open; sh->ge = o->gap_extend; sh->want_cigar = o->want_cigar != 0;
    const int64_t workspace = o->workspace_bytes > 0 ? o->workspace_bytes : (int64_t)1 << 30;
    pairs->resize((size_t)n);
    int first = 0;
    int64_t share = 0;
    for (int k = 0; k < n; ++k) {
        Pair& p = (*pairs)[(size_t)k];
        const int64_t m = q_off[k + 1] - q_off[k], nn = refs.len[(size_t)k];
        p.q_off = q_off[k] - q_off[0]; p.r_off = refs.start[(size_t)k];
        p.m = (int32_t)m; p.n = (int32_t)nn;
        p.ws_off = -1; p.cig_off = sh->cig_cap; p.cig_cap = 0;
        const bool kernel = m > 0 && nn > 0;
        sh->nempty += !kernel;
        const int64_t need = own(k, p, kernel);
        if (sh->want_cigar) {
            p.cig_cap = (int32_t)std::min<int64_t>(m + nn, 2 * std::min(m, nn) + 1);      // runs alternate: no CIGAR has more
            sh->cig_cap += p.cig_cap;
        }
        if (sh->want_cigar && kernel) {
            sh->max_pair_ws = std::max(sh->max_pair_ws, need);
            if (need > workspace)
                return fail(CLH_E_CAPACITY, me + "pair " + std::to_string(k) + " alone needs " + std::to_string(need) + " bytes of workspace for the decisions of its " +
                                            cells(p) + ", workspace_bytes is " + std::to_string(workspace));
            if (share + need > workspace) { sh->shares.push_back({first, k - first}); first = k; share = 0; }
            p.ws_off = share; share += need;
            sh->ws_bytes = std::max(sh->ws_bytes, share);
        }
    }
    if (n > first) sh->shares.push_back({first, n - first});
    return 0;
}

// the plan takes over what was planned and uploads what both kinds have; false: a block is missing
template <typename Pair>
static bool pairs_upload(clh_pairs_plan* pl, PairsShape* sh, const std::vector<Pair>& pairs, const int8_t* q, const int64_t* q_off, const PairsRefs& refs,
                         const int8_t* mat)
{
    static_cast<PairsShape&>(*pl) = std::move(*sh);
    const int n = pl->n;
    const int64_t tq = n ? q_off[n] - q_off[0] : 0;
    pl->d_q = pl->upload(q ? q + q_off[0] : nullptr, (size_t)tq);
    pl->d_r = refs.genome ? pl->alloc((size_t)refs.total) : pl->upload(refs.r ? refs.r + refs.r_off[0] : nullptr, (size_t)refs.total);
    pl->d_pairs = pl->upload(pairs.data(), sizeof(Pair) * pairs.size());
    pl->d_mat = pl->upload(mat, (size_t)pl->n_mat * pl->n_mat);
    pl->d_ws = pl->alloc((size_t)std::max<int64_t>(pl->ws_bytes, 1));
    pl->d_rows = pl->alloc(32 * (size_t)std::max(n, 1));
    pl->d_cig = pl->alloc(sizeof(uint32_t) * (size_t)std::max<int64_t>(pl->cig_cap, 1));
    return pl->d_q && pl->d_r && pl->d_pairs && pl->d_mat && pl->d_ws && pl->d_rows && pl->d_cig;
}

// the windows form: the device fills the plan's reference buffer from the resident genome, once, here; the plan is ready on return
static int pairs_gather(const std::string& me, clh_pairs_plan* pl, const PairsRefs& refs)
{
    if (!refs.genome) return 0;
    const int n = pl->n;
    std::vector<clh::GatherTask> tasks((size_t)n);
    std::vector<int32_t> tile_task;
    int64_t tiles = 0;
    for (int k = 0; k < n; ++k) {
        tasks[(size_t)k] = clh::GatherTask{refs.win_off[k], refs.start[(size_t)k], (int32_t)refs.len[(size_t)k], (int32_t)refs.win_flags[k], tiles};
        const int64_t nt = clh::gather_tiles(refs.len[(size_t)k]);
        tile_task.insert(tile_task.end(), (size_t)nt, (int32_t)k);
        tiles += nt;
    }
    if (!tiles) return 0;
    void* d_tasks = pl->upload(tasks.data(), sizeof(clh::GatherTask) * tasks.size());
    void* d_tiles = pl->upload(tile_task.data(), sizeof(int32_t) * tile_task.size());
    if (!d_tasks || !d_tiles) return fail(CLH_E_HIP, me + "out of device memory or upload failed for the gather's tasks");
    hipStream_t st = pl->ctx->stream;
    hipEvent_t ev[2];
    for (auto& e : ev) HIPCHK(pl->event(&e));
    HIPCHK(hipEventRecord(ev[0], st));
    HIPCHK(clh::launch_genome_gather((const uint8_t*)refs.genome->d_codes, refs.genome->len, (const clh::GatherTask*)d_tasks, n, (const int32_t*)d_tiles, tiles,
                                     (int8_t*)pl->d_r, refs.total, st));
    HIPCHK(hipEventRecord(ev[1], st));
    HIPCHK(hipStreamSynchronize(st));      // the tables go back to the allocator, and a run may use another stream
    HIPCHK(hipEventElapsedTime(&pl->gather_ms, ev[0], ev[1]));
    for (int k = 0; k < n; ++k) pl->gather_letters += refs.len[(size_t)k];
    pl->free_block(d_tasks); pl->free_block(d_tiles);
    return 0;
}

static int pairs_gather_timing(const std::string& me, const clh_pairs_plan* pl, float* ms, int64_t* letters)
{
    if (!pl || !ms || !letters) return fail(CLH_E_ARG, me + "null argument");
    if (pl->gather_ms < 0) return fail(CLH_E_ARG, me + "no gather to time: the plan's references are strings, or its windows hold no letter");
    *ms = pl->gather_ms; *letters = pl->gather_letters;
    return 0;
}

// the start of a run of either kind; every row starts as "unwritten": what a kernel did not store is reported by fetch, never returned
static int pairs_begin_run(clh_pairs_plan* pl, void* stream_, hipStream_t* st)
{
    if (int rc = pl->begin_run(stream_, st)) return rc;
    if (pl->n) HIPCHK(hipMemsetAsync(pl->d_rows, 0x80, 32 * (size_t)pl->n, *st));
    return 0;
}

// what the programme gives when one side has no letter: the boundary itself
// (intron >= 0: the spliced programme, whose row 0 is one deletion or, where that is dearer, one intron)
template <typename Row>
static void en_empty_side(int mode, int m, int n, const PairsShape& sh, Row* row, uint32_t* op, int64_t intron = -1)
{
    *op = 0;
    row->score = 0; row->ref_begin = 0; row->ref_end = -1; row->query_begin = 0; row->query_end = -1;
    if (n > 0 && mode == CLH_ENDS_GLOBAL) {
        const bool as_intron = intron >= 0 && intron < sh.gap(n);
        row->score = (int32_t)-(as_intron ? intron : sh.gap(n)); row->ref_end = n - 1; *op = ((uint32_t)n << 4) | (as_intron ? 3u : 2u);
    }
    if (mode == CLH_ENDS_EXTEND) return;                       // the best cell of a boundary that only loses is (0, 0)
    if (m > 0 && mode != CLH_ENDS_OVERLAP) { row->score = (int32_t)-sh.gap(m); row->query_end = m - 1; *op = ((uint32_t)m << 4) | 1u; }
    if (m > 0 && mode == CLH_ENDS_OVERLAP) { row->query_begin = m; row->query_end = m - 1; }
}

// fetch of either kind (`kind`: "ends" / "band", for the messages): the rows and CIGARs of the last run, the rows of pairs with an
// empty side stated here.  more(pair, row) is called once the fields of clh_ends_row but the CIGAR's are in place, for what a kind adds.
template <typename Plan, typename Row, typename More>
static int pairs_fetch(const std::string& kind, Plan* pl, Row* rows, uint32_t* cigar, int64_t cigar_cap, int64_t* cigar_used, More more)
{
    const std::string me = "clh_" + kind + "_plan_fetch: ";
    if (!pl || (!rows && pl->n > 0)) return fail(CLH_E_ARG, me + "null argument");
    if (!pl->ran) return fail(CLH_E_ARG, "clh_" + kind + "_plan_fetch before clh_" + kind + "_plan_run");
    if (cigar_used) *cigar_used = 0;
    if (!pl->n) return 0;
    HIPCHK(hipSetDevice(pl->ctx->device));
    HIPCHK(hipStreamSynchronize(pl->last_stream));
    std::vector<int32_t> raw(8 * (size_t)pl->n);
    HIPCHK(hipMemcpy(raw.data(), pl->d_rows, 32 * (size_t)pl->n, hipMemcpyDeviceToHost));
    std::vector<uint32_t> ops;
    if (pl->want_cigar && pl->cig_cap) {
        ops.resize((size_t)pl->cig_cap);
        HIPCHK(hipMemcpy(ops.data(), pl->d_cig, sizeof(uint32_t) * ops.size(), hipMemcpyDeviceToHost));
    }
    int64_t used = 0, unwritten = 0, nowalk = 0, first_bad = -1;
    for (int k = 0; k < pl->n; ++k) {
        const auto& p = pl->pairs[(size_t)k];
        const int32_t* w = raw.data() + 8 * (size_t)k;
        Row& out = rows[k];
        uint32_t one = 0;
        const uint32_t* src = nullptr;
        int len = 0;
        if (p.m == 0 || p.n == 0) {
            en_empty_side(pl->mode, p.m, p.n, *pl, &out, &one, pl->row0_intron.empty() ? -1 : pl->row0_intron[(size_t)k]);
            if (one) { src = &one; len = 1; }
        } else {
            bool bad = false;
            for (int f = 0; f < 8; ++f) bad |= w[f] == clh::kEnUnwritten;
            if (bad) { ++unwritten; if (first_bad < 0) first_bad = k; continue; }
            if (w[7] != 0 || w[5] < 0 || w[5] > p.cig_cap) { ++nowalk; if (first_bad < 0) first_bad = k; continue; }
            out.score = w[0]; out.ref_begin = w[1]; out.ref_end = w[2]; out.query_begin = w[3]; out.query_end = w[4];
            src = ops.data() + p.cig_off; len = w[5];
        }
        more(p, out);
        out.cigar_len = 0; out.cigar_off = -1;
        if (pl->want_cigar) {
            if (cigar && used + len > cigar_cap) return fail(CLH_E_CAPACITY, me + "cigar_cap too small");
            out.cigar_len = len; out.cigar_off = used;
            if (cigar && len) memcpy(cigar + used, src, sizeof(uint32_t) * (size_t)len);
            used += len;
        }
    }
    if (cigar_used) *cigar_used = used;
    if (unwritten || nowalk)
        return fail(CLH_E_HIP, me + "the kernels left " + std::to_string(unwritten) + " rows unwritten and " + std::to_string(nowalk) +
                                   " without their walk (first: pair " + std::to_string(first_bad) + ")");
    return 0;
}

// a one-shot batch of either kind over the plan its create call returned (null: it has failed): run, fetch, delete
template <typename Plan, typename Row>
static int pairs_batch(Plan* pl, int (*run)(Plan*, void*), int (*fetch)(Plan*, Row*, uint32_t*, int64_t, int64_t*), Row* rows, uint32_t* cigar,
                       int64_t cigar_cap, int64_t* cigar_used)
{
    if (!pl) return g_code;
    int rc = run(pl, nullptr);
    if (!rc) rc = fetch(pl, rows, cigar, cigar_cap, cigar_used);
    delete pl;
    return rc;
}

// ---------------------------------------------------------------------------------------------------------------
// K1g: end-anchored affine-gap alignment of pairs -- global, semiglobal, overlap, prefix, extend (ssw_ends.hip)
// ---------------------------------------------------------------------------------------------------------------
struct clh_ends_plan : clh_pairs_plan {
    using clh_pairs_plan::clh_pairs_plan;
    std::vector<clh::EnPair> pairs;
    int64_t hand_words = 0;
    void* d_hand = nullptr;
    bool recompute = false;                       // CIGARs by the recompute route (CLH_ENDS_CIGAR_RECOMPUTE): a share's block holds EnKept blocks
    std::vector<int> share_rounds;                // recompute: per share, the greatest chunk count among its pairs
    void *d_site = nullptr, *d_strand = nullptr;  // spliced: the site costs of both strands and the pairs' strands (null: all +)
};

extern "C" void clh_ends_plan_destroy(clh_ends_plan* pl) { delete pl; }

// a lane's row of decisions: 4 bits per cell with one piece, a byte per cell with two
static int64_t en_ws_bytes(int64_t m, int64_t n, int pieces)
{
    const int64_t nch = (n + clh::kEnChunk - 1) / clh::kEnChunk;
    const int64_t llast = (n - (nch - 1) * clh::kEnChunk + clh::kEnCpl - 1) / clh::kEnCpl;
    return (4 * pieces * m * (64 * (nch - 1) + llast) + 15) & ~(int64_t)15;
}

// the cost of the dinucleotide (x, y) as the reference reads it, from the table ssw_ends.hip's spliced kernels take (clh_device.h)
static int64_t sp_site(const int32_t* site, int soff, int which, int x, int y)
{
    return site[((x | y) > 3 || (x | y) < 0) ? clh::kSpOther : soff + which + 4 * x + y];
}

// the table of both strands that ssw_ends.hip's spliced kernels and seed_junction.hip take (clh_device.h)
static void sp_table(const clh_splice* sp, int32_t* site)
{
    for (int x = 0; x < 4; ++x)
        for (int y = 0; y < 4; ++y) {      // strand -: the transcript reads the complement of (y, x)
            site[4 * x + y] = sp->donor[4 * x + y]; site[16 + 4 * x + y] = sp->acceptor[4 * x + y];
            site[32 + 4 * x + y] = sp->acceptor[4 * (3 - y) + (3 - x)]; site[48 + 4 * x + y] = sp->donor[4 * (3 - y) + (3 - x)];
        }
    site[clh::kSpOther] = sp->other;
}

// what the spliced create refuses beyond pairs_check_opts, and the table of both strands -> 0, or the code
static int sp_check(const std::string& me, const clh_ends_opts* o, const clh_splice* sp, const int8_t* strand, int32_t n, int32_t* site, int64_t* site_max)
{
    if (!sp) return fail(CLH_E_ARG, me + "null splice");
    bool dna = o->n_mat == 5;
    for (int a = 0; dna && a < 5; ++a)
        for (int b = 0; b < 5; ++b) {
            const int want = (a == 4 || b == 4) ? 0 : (a == b ? o->mat[0] : o->mat[1]);
            dna = dna && o->mat[a * 5 + b] == want;
        }
    if (!dna)
        return fail(CLH_E_UNSUPPORTED, me + "spliced alignment takes the DNA match / mismatch matrix alone (5 x 5: one match score, one mismatch score, 0 against N); "
                                            "substitution matrices over other alphabets are not built");
    int64_t dmax = sp->other, amax = sp->other;
    bool neg = sp->intron_open < 0 || sp->other < 0;
    for (int k = 0; k < 16; ++k) {
        neg = neg || sp->donor[k] < 0 || sp->acceptor[k] < 0;
        dmax = std::max<int64_t>(dmax, sp->donor[k]); amax = std::max<int64_t>(amax, sp->acceptor[k]);
    }
    if (neg) return fail(CLH_E_ARG, me + "intron_open, the donor and acceptor costs and `other` must not be negative");
    if (strand)
        for (int k = 0; k < n; ++k)
            if (strand[k] != 1 && strand[k] != -1) return fail(CLH_E_ARG, me + "pair " + std::to_string(k) + ": strand must be +1 or -1, got " + std::to_string((int)strand[k]));
    *site_max = (int64_t)sp->intron_open + dmax + amax;
    sp_table(sp, site);
    return 0;
}

// the creates of K1g; g2: the second piece, null for one piece; sp: intron gaps (clh_splice) with the pairs' strands, null for none
static clh_ends_plan* en_create(const std::string& me, clh_ctx* ctx, int32_t n, const int8_t* q, const int64_t* q_off, PairsRefs refs,
                                const clh_ends_opts* o, const clh_gap2* g2, const clh_splice* sp = nullptr, const int8_t* strand = nullptr, bool spliced = false)
{
    if (pairs_check_opts(me, ctx, n, q_off, refs.off_arg(q_off), o, nullptr, g2)) return nullptr;
    if (pairs_ref_spans(me, n, o->n_mat, &refs)) return nullptr;
    const int pieces = (g2 || spliced) ? 2 : 1;       // the spliced kernel stores a byte per cell and hands three values on, as two pieces do
    int64_t splus;
    int64_t smax = pairs_scan_matrix(o, &splus, g2);
    int32_t site[clh::kSpSites];
    if (spliced) {
        int64_t site_max = 0;
        if (sp_check(me, o, sp, strand, n, site, &site_max)) return nullptr;
        smax = std::max(smax, site_max);
    }
    for (int k = 0; k < n; ++k) {
        const int64_t m = q_off[k + 1] - q_off[k], nn = refs.len[(size_t)k];
        if (m < 0 || nn < 0) { fail(CLH_E_ARG, me + "offsets must ascend"); return nullptr; }
        if ((m > 0 && !q) || (nn > 0 && !refs.genome && !refs.r)) { fail(CLH_E_ARG, me + "null argument"); return nullptr; }
        if (m + nn >= ((int64_t)1 << 30) || (m + nn) * smax >= ((int64_t)1 << 30)) {
            fail(CLH_E_ARG, me + "pair " + std::to_string(k) + ": (m + n) * max(|s|, " +
                                (spliced ? "gap_open, gap_extend, intron_open + dmax + amax" : g2 ? "gap_open, gap_extend, gap_open2, gap_extend2" : "gap_open, gap_extend") +
                                ") = " + std::to_string(m + nn) + " * " +
                                std::to_string(smax) + " reaches 2^30, the score range of the int32 cells");
            return nullptr;
        }
    }
    if (pairs_check_codes(me, n, q, q_off, refs.r, refs.r_off, o->n_mat)) return nullptr;
    PairsShape shape;
    if (g2) { shape.pieces = 2; shape.go2 = g2->gap_open2; shape.ge2 = g2->gap_extend2; }
    // spliced, global, no query letter: the reference as one intron, from its first two and last two letters (`edge`: 0, 1, n - 2, n - 1)
    auto row0_intron = [&](int k, int64_t nn, const int8_t* edge) {
        const int soff = (strand && strand[k] < 0) ? 32 : 0;
        return (int64_t)sp->intron_open + sp_site(site, soff, 0, edge[0], nn > 1 ? edge[1] : 4) + sp_site(site, soff, 16, nn > 1 ? edge[2] : 4, edge[3]);
    };
    if (spliced) {
        shape.spliced = true; shape.io = sp->intron_open;
        shape.row0_intron.assign((size_t)n, -1);
        for (int k = 0; k < n && o->mode == CLH_ENDS_GLOBAL && !refs.genome; ++k) {
            const int64_t m = q_off[k + 1] - q_off[k], nn = refs.len[(size_t)k];
            if (m != 0 || nn == 0) continue;
            const int8_t* rk = refs.r + refs.r_off[k];
            const int8_t edge[4] = {rk[0], nn > 1 ? rk[1] : (int8_t)4, nn > 1 ? rk[nn - 2] : (int8_t)4, rk[nn - 1]};
            shape.row0_intron[(size_t)k] = row0_intron(k, nn, edge);
        }
    }
    std::vector<clh::EnPair> pairs;
    int64_t hand_words = 0;
    const bool recompute = o->want_cigar == CLH_ENDS_CIGAR_RECOMPUTE;
    if (pairs_cut_shares(me, o, n, q_off, refs, &shape, &pairs,
            [&](int, clh::EnPair& p, bool kernel) {
                p.pad = 0; p.hand_off = -1;
                // recompute: every chunk's last column is kept in the pair's block of the workspace, beside one chunk's plane and the walk's record
                if (recompute) return kernel ? clh::EnKept(p.m, p.n, 1 + pieces, 4 * pieces).total : 0;
                // two buffers of H and one E per piece of the last column, per row
                if (kernel && p.n > clh::kEnChunk) { p.hand_off = hand_words; hand_words += 2 * (1 + pieces) * (((int64_t)p.m + 63) & ~(int64_t)63); }
                return kernel ? en_ws_bytes(p.m, p.n, pieces) : 0;
            },
            [&](const clh::EnPair& p) {
                return std::to_string(p.m) + " x " + std::to_string(p.n) + " cells" +
                       (recompute ? std::string(" (recompute route: kept chunk columns, one chunk's plane and the walk's record)") : std::string());
            }))
        return nullptr;
    if (hipSetDevice(ctx->device) != hipSuccess) { fail(CLH_E_HIP, "hipSetDevice failed"); return nullptr; }
    clh_ends_plan* pl = new clh_ends_plan(ctx);
    pl->hand_words = hand_words;
    const bool ok = pairs_upload(pl, &shape, pairs, q, q_off, refs, o->mat);
    pl->pairs.swap(pairs);
    pl->recompute = recompute;
    for (const auto& sh : pl->shares) {
        int64_t nmax = 0;
        for (int k = sh.first; k < sh.first + sh.second; ++k)
            if (pl->pairs[(size_t)k].m > 0) nmax = std::max<int64_t>(nmax, pl->pairs[(size_t)k].n);
        pl->share_rounds.push_back((int)((nmax + clh::kEnChunk - 1) / clh::kEnChunk));
    }
    pl->d_hand = pl->alloc(sizeof(int32_t) * (size_t)std::max<int64_t>(pl->hand_words, 1));
    bool sp_ok = true;
    if (spliced) {
        pl->d_site = pl->upload(site, sizeof site);
        if (strand && n) pl->d_strand = pl->upload(strand, (size_t)n);
        sp_ok = pl->d_site && (!strand || !n || pl->d_strand);
    }
    if (!ok || !pl->d_hand || !sp_ok) {
        fail(CLH_E_HIP, "out of device memory or upload failed while building the ends plan");
        delete pl; return nullptr;
    }
    if (pairs_gather(me, pl, refs)) { delete pl; return nullptr; }
    // the windows form of row0_intron: the same four letters, read back from what the gather wrote
    for (int k = 0; k < n && spliced && o->mode == CLH_ENDS_GLOBAL && refs.genome; ++k) {
        const int64_t nn = pl->pairs[(size_t)k].n;
        if (pl->pairs[(size_t)k].m != 0 || nn == 0) continue;
        const int8_t* dk = (const int8_t*)pl->d_r + pl->pairs[(size_t)k].r_off;
        int8_t edge[4] = {4, 4, 4, 4};
        const int64_t head = std::min<int64_t>(nn, 2);
        if (hipMemcpy(edge, dk, (size_t)head, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(edge + 4 - head, dk + nn - head, (size_t)head, hipMemcpyDeviceToHost) != hipSuccess) {
            fail(CLH_E_HIP, me + "reading back the window's edge letters failed");
            delete pl; return nullptr;
        }
        pl->row0_intron[(size_t)k] = row0_intron(k, nn, edge);
    }
    return pl;
}

extern "C" clh_ends_plan* clh_ends_plan_create(clh_ctx* ctx, int32_t n, const int8_t* q, const int64_t* q_off, const int8_t* r, const int64_t* r_off,
                                               const clh_ends_opts* o)
{
    return en_create("clh_ends_plan_create: ", ctx, n, q, q_off, refs_strings(r, r_off), o, nullptr);
}

extern "C" clh_ends_plan* clh_ends_plan_create_gap2(clh_ctx* ctx, int32_t n, const int8_t* q, const int64_t* q_off, const int8_t* r, const int64_t* r_off,
                                                    const clh_ends_opts* o, const clh_gap2* gap2)
{
    if (!gap2) return clh_ends_plan_create(ctx, n, q, q_off, r, r_off, o);
    return en_create("clh_ends_plan_create_gap2: ", ctx, n, q, q_off, refs_strings(r, r_off), o, gap2);
}

extern "C" clh_ends_plan* clh_ends_plan_create_spliced(clh_ctx* ctx, int32_t n, const int8_t* q, const int64_t* q_off, const int8_t* r, const int64_t* r_off,
                                                       const clh_ends_opts* o, const clh_splice* splice, const int8_t* strand)
{
    return en_create("clh_ends_plan_create_spliced: ", ctx, n, q, q_off, refs_strings(r, r_off), o, nullptr, splice, strand, true);
}

// K1g on windows of the resident genome: gap2 for two pieces, splice (with strand, which may be null) for introns, both null for neither
extern "C" clh_ends_plan* clh_ends_plan_create_windows(clh_genome* genome, int32_t n, const int8_t* q, const int64_t* q_off, const int64_t* win_off,
                                                       const int32_t* win_len, const uint8_t* win_flags, const clh_ends_opts* o, const clh_gap2* gap2,
                                                       const clh_splice* splice, const int8_t* strand)
{
    const std::string me = "clh_ends_plan_create_windows: ";
    if (!genome) { fail(CLH_E_ARG, me + "null genome"); return nullptr; }
    if (gap2 && splice) { fail(CLH_E_UNSUPPORTED, me + "two-piece gap costs together with introns are not built"); return nullptr; }
    if (strand && !splice) { fail(CLH_E_ARG, me + "strand comes with splice"); return nullptr; }
    return en_create(me, genome->ctx, n, q, q_off, refs_windows(genome, win_off, win_len, win_flags), o, gap2, splice, strand, splice != nullptr);
}

extern "C" int clh_ends_plan_run(clh_ends_plan* pl, void* stream_)
{
    if (!pl) return fail(CLH_E_ARG, "clh_ends_plan_run: null argument");
    hipStream_t st;
    if (int rc = pairs_begin_run(pl, stream_, &st)) return rc;
    clh::En2Params p;
    p.go2 = pl->go2; p.ge2 = pl->ge2;
    p.qry = (const int8_t*)pl->d_q; p.ref = (const int8_t*)pl->d_r;
    p.pairs = (const clh::EnPair*)pl->d_pairs; p.npairs = pl->n;
    p.mat = (const int8_t*)pl->d_mat; p.n_mat = pl->n_mat;
    p.go = pl->go; p.ge = pl->ge; p.mode = pl->mode;
    p.hand = (int32_t*)pl->d_hand; p.hand_cap = pl->hand_words;
    p.ws = (uint8_t*)pl->d_ws; p.ws_cap = pl->ws_bytes;
    p.rows = (int32_t*)pl->d_rows;
    p.cigar = (uint32_t*)pl->d_cig; p.cigar_cap = pl->cig_cap;
    // in stream order: a share's walk has read the workspace before the next share fills it
    // (recompute: a share is the keeping score pass and then, chunk after chunk leftwards, the tile form and a round of the walk)
    auto run_shares = [&](const auto& prm, auto launch, auto launch_walk, auto launch_retrace) -> int {
        for (size_t s = 0; s < pl->shares.size(); ++s) {
            const auto& sh = pl->shares[s];
            if (pl->want_cigar && pl->recompute) { HIPCHK(launch_retrace(prm, sh.first, sh.second, pl->share_rounds[s], st)); continue; }
            HIPCHK(launch(prm, pl->want_cigar, sh.first, sh.second, st));
            if (pl->want_cigar) HIPCHK(launch_walk(prm, sh.first, sh.second, st));
        }
        return 0;
    };
    int rc;
    if (pl->spliced) {      // K1g's argument block with the site costs behind it
        clh::SpParams sp;
        static_cast<clh::EnParams&>(sp) = p;
        sp.io = pl->io; sp.site = (const int32_t*)pl->d_site; sp.strand = (const int8_t*)pl->d_strand;
        rc = run_shares(sp, clh::launch_ssw_spliced, clh::launch_ssw_spliced_walk, clh::launch_ssw_spliced_retrace);
    }
    else if (pl->pieces == 2) rc = run_shares(p, clh::launch_ssw_ends2, clh::launch_ssw_ends2_walk, clh::launch_ssw_ends2_retrace);
    else rc = run_shares(p, clh::launch_ssw_ends, clh::launch_ssw_ends_walk, clh::launch_ssw_ends_retrace);      // the one-piece launchers take the block's base
    return rc ? rc : pl->end_run();
}

extern "C" int clh_ends_plan_fetch(clh_ends_plan* pl, clh_ends_row* rows, uint32_t* cigar, int64_t cigar_cap, int64_t* cigar_used)
{
    return pairs_fetch("ends", pl, rows, cigar, cigar_cap, cigar_used, [](const clh::EnPair&, clh_ends_row&) {});
}

extern "C" int clh_ends_plan_timing(clh_ends_plan* pl, float* ms)
{
    if (!pl || !ms || !pl->ran) return fail(CLH_E_ARG, "clh_ends_plan_timing: no run to time");
    return pl->elapsed(ms);
}

extern "C" int clh_ends_plan_gather_timing(clh_ends_plan* pl, float* ms, int64_t* letters)
{
    return pairs_gather_timing("clh_ends_plan_gather_timing: ", pl, ms, letters);
}

extern "C" int clh_ends_plan_info(clh_ends_plan* pl, int64_t* out)
{
    if (!pl || !out) return fail(CLH_E_ARG, "clh_ends_plan_info: null argument");
    out[0] = clh::kEnCpl; out[1] = clh::kEnChunk; out[2] = (int64_t)pl->shares.size(); out[3] = pl->ws_bytes;
    out[4] = pl->max_pair_ws; out[5] = pl->n - pl->nempty; out[6] = pl->nempty; out[7] = pl->cig_cap;
    return 0;
}

extern "C" int clh_ends_batch(clh_ctx* ctx, int32_t n, const int8_t* q, const int64_t* q_off, const int8_t* r, const int64_t* r_off, const clh_ends_opts* opts,
                              clh_ends_row* rows, uint32_t* cigar, int64_t cigar_cap, int64_t* cigar_used)
{
    return pairs_batch(clh_ends_plan_create(ctx, n, q, q_off, r, r_off, opts), clh_ends_plan_run, clh_ends_plan_fetch, rows, cigar, cigar_cap, cigar_used);
}

extern "C" int clh_ends_batch_gap2(clh_ctx* ctx, int32_t n, const int8_t* q, const int64_t* q_off, const int8_t* r, const int64_t* r_off, const clh_ends_opts* opts,
                                   const clh_gap2* gap2, clh_ends_row* rows, uint32_t* cigar, int64_t cigar_cap, int64_t* cigar_used)
{
    return pairs_batch(clh_ends_plan_create_gap2(ctx, n, q, q_off, r, r_off, opts, gap2), clh_ends_plan_run, clh_ends_plan_fetch, rows, cigar, cigar_cap, cigar_used);
}

extern "C" int clh_ends_batch_spliced(clh_ctx* ctx, int32_t n, const int8_t* q, const int64_t* q_off, const int8_t* r, const int64_t* r_off, const clh_ends_opts* opts,
                                     const clh_splice* splice, const int8_t* strand, clh_ends_row* rows, uint32_t* cigar, int64_t cigar_cap, int64_t* cigar_used)
{
    return pairs_batch(clh_ends_plan_create_spliced(ctx, n, q, q_off, r, r_off, opts, splice, strand), clh_ends_plan_run, clh_ends_plan_fetch, rows, cigar, cigar_cap, cigar_used);
}

// ---------------------------------------------------------------------------------------------------------------
// K1gb: K1g's global, semiglobal, prefix and extend programmes over a band of diagonals per pair (ssw_band.hip)
// ---------------------------------------------------------------------------------------------------------------
struct clh_band_plan : clh_pairs_plan {
    using clh_pairs_plan::clh_pairs_plan;
    int64_t splus = 0;                            // max(0, greatest matrix entry): what an M column can add at most
    std::vector<clh::BdPair> pairs;
    std::vector<int32_t> order;                   // pair indices filed by share, then by class
    struct classes_t { int cfirst[clh::kBdClasses], ccount[clh::kBdClasses]; };
    std::vector<classes_t> share_classes;         // per share: where the pairs of each class stand in `order`
    int64_t max_width = 0, nclass[clh::kBdClasses] = {0, 0, 0};
    void* d_order = nullptr;
};

extern "C" void clh_band_plan_destroy(clh_band_plan* pl) { delete pl; }

// both creates of K1gb; g2: the second piece, null for one piece
static clh_band_plan* bd_create(const std::string& me, clh_ctx* ctx, int32_t n, const int8_t* q, const int64_t* q_off, PairsRefs refs,
                                const int32_t* diag, const clh_band_opts* bo, const clh_gap2* g2)
{
    clh_ends_opts shared;                                                      // the fields the two share (the static_asserts above)
    if (bo) memcpy(&shared, bo, sizeof shared);
    const clh_ends_opts* o = bo ? &shared : nullptr;
    if (pairs_check_opts(me, ctx, n, q_off, refs.off_arg(q_off), o, bo ? &bo->band : nullptr, g2)) return nullptr;
    if (pairs_ref_spans(me, n, o->n_mat, &refs)) return nullptr;
    const int pieces = g2 ? 2 : 1;
    int64_t splus;
    const int64_t smax = pairs_scan_matrix(o, &splus, g2);
    const bool global = o->mode == CLH_ENDS_GLOBAL;
    const bool anchored = o->mode == CLH_ENDS_PREFIX || o->mode == CLH_ENDS_EXTEND;      // the far end is free: n - m plays no part in the band
    std::vector<std::pair<int32_t, int32_t>> bands((size_t)n);
    for (int k = 0; k < n; ++k) {
        const int64_t m = q_off[k + 1] - q_off[k], nn = refs.len[(size_t)k];
        const std::string pk = me + "pair " + std::to_string(k) + ": ";
        if (m < 0 || nn < 0) { fail(CLH_E_ARG, me + "offsets must ascend"); return nullptr; }
        if ((m > 0 && !q) || (nn > 0 && !refs.genome && !refs.r)) { fail(CLH_E_ARG, me + "null argument"); return nullptr; }
        const int64_t span = m + nn + 2 * clh::kBdMaxWidth;
        if (span >= ((int64_t)1 << 29) || span * smax >= ((int64_t)1 << 29)) {
            fail(CLH_E_ARG, pk + "(m + n + " + std::to_string(2 * clh::kBdMaxWidth) + ") * max(|s|, " + (g2 ? "gap_open, gap_extend, gap_open2, gap_extend2" : "gap_open, gap_extend") +
                                ") = " + std::to_string(span) + " * " +
                                std::to_string(smax) + " reaches 2^29, the score range the banded int32 cells keep apart from minus infinity");
            return nullptr;
        }
        int64_t lo, hi;
        if (diag) { lo = (int64_t)diag[k] - bo->band; hi = (int64_t)diag[k] + bo->band; }
        else if (anchored) { lo = -(int64_t)bo->band; hi = bo->band; }
        else { lo = std::min<int64_t>(0, nn - m) - bo->band; hi = std::max<int64_t>(0, nn - m) + bo->band; }
        const std::string bt = "the band [" + std::to_string(lo) + ", " + std::to_string(hi) + "] of the " + std::to_string(m) + " x " + std::to_string(nn) + " pair ";
        if (global && (lo > std::min<int64_t>(0, nn - m) || hi < std::max<int64_t>(0, nn - m))) {
            fail(CLH_E_ARG, pk + bt + "misses (0, 0) or (m, n): a global band holds the diagonals 0 and n - m = " + std::to_string(nn - m));
            return nullptr;
        }
        if (anchored && (lo > 0 || hi < 0)) {
            fail(CLH_E_ARG, pk + bt + "misses (0, 0): a start-anchored band holds the diagonal 0");
            return nullptr;
        }
        if (o->mode == CLH_ENDS_PREFIX && lo > nn - m) {
            fail(CLH_E_ARG, pk + bt + "has no end cell on row m (lo > n - m = " + std::to_string(nn - m) + ")");
            return nullptr;
        }
        if (!global && !anchored && (hi < 0 || lo > nn - m)) {
            fail(CLH_E_ARG, pk + bt + "has no start cell on row 0 (hi < 0) or no end cell on row m (lo > n - m = " + std::to_string(nn - m) + ")");
            return nullptr;
        }
        lo = std::max(lo, -m); hi = std::min(hi, nn);
        if (hi - lo + 1 > clh::kBdMaxWidth) {
            fail(CLH_E_CAPACITY, pk + "the clipped band [" + std::to_string(lo) + ", " + std::to_string(hi) + "] holds " + std::to_string(hi - lo + 1) +
                                 " diagonals, more than " + std::to_string(clh::kBdMaxWidth) + "; clh_ends_plan_create takes such pairs over the full matrix");
            return nullptr;
        }
        bands[(size_t)k] = {(int32_t)lo, (int32_t)hi};
    }
    if (pairs_check_codes(me, n, q, q_off, refs.r, refs.r_off, o->n_mat)) return nullptr;
    PairsShape shape;
    if (g2) { shape.pieces = 2; shape.go2 = g2->gap_open2; shape.ge2 = g2->gap_extend2; }
    std::vector<clh::BdPair> pairs;
    int64_t max_width = 0, nclass[clh::kBdClasses] = {0, 0, 0};
    if (pairs_cut_shares(me, o, n, q_off, refs, &shape, &pairs,
            [&](int k, clh::BdPair& p, bool kernel) -> int64_t {
                p.lo = bands[(size_t)k].first; p.hi = bands[(size_t)k].second; p.cls = -1;
                if (!kernel) return 0;
                const int64_t B = (int64_t)p.hi - p.lo + 1;
                p.cls = 0;
                while (B > 64 * clh::kBdCpl[p.cls]) ++p.cls;
                ++nclass[p.cls];
                max_width = std::max(max_width, B);
                const int cpl = clh::kBdCpl[p.cls];
                return ((int64_t)p.m * ((B + cpl - 1) / cpl) * (cpl / 2) * pieces + 15) & ~(int64_t)15;      // half a byte per cell and piece
            },
            [](const clh::BdPair& p) { return std::to_string(p.m) + " rows of " + std::to_string((int64_t)p.hi - p.lo + 1) + " diagonals"; }))
        return nullptr;
    std::vector<int32_t> order;
    std::vector<clh_band_plan::classes_t> share_classes(shape.shares.size());
    for (size_t s = 0; s < shape.shares.size(); ++s)
        for (int c = 0; c < clh::kBdClasses; ++c) {
            const auto& sh = shape.shares[s];
            share_classes[s].cfirst[c] = (int)order.size();
            for (int k = sh.first; k < sh.first + sh.second; ++k)
                if (pairs[(size_t)k].cls == c) order.push_back(k);
            share_classes[s].ccount[c] = (int)order.size() - share_classes[s].cfirst[c];
        }
    if (hipSetDevice(ctx->device) != hipSuccess) { fail(CLH_E_HIP, "hipSetDevice failed"); return nullptr; }
    clh_band_plan* pl = new clh_band_plan(ctx);
    pl->splus = splus; pl->max_width = max_width;
    for (int c = 0; c < clh::kBdClasses; ++c) pl->nclass[c] = nclass[c];
    const bool ok = pairs_upload(pl, &shape, pairs, q, q_off, refs, o->mat);
    pl->pairs.swap(pairs); pl->order.swap(order); pl->share_classes.swap(share_classes);
    pl->d_order = pl->upload(pl->order.data(), sizeof(int32_t) * pl->order.size());
    if (!ok || !pl->d_order) {
        fail(CLH_E_HIP, "out of device memory or upload failed while building the band plan");
        delete pl; return nullptr;
    }
    if (pairs_gather(me, pl, refs)) { delete pl; return nullptr; }
    return pl;
}

extern "C" clh_band_plan* clh_band_plan_create(clh_ctx* ctx, int32_t n, const int8_t* q, const int64_t* q_off, const int8_t* r, const int64_t* r_off,
                                               const int32_t* diag, const clh_band_opts* bo)
{
    return bd_create("clh_band_plan_create: ", ctx, n, q, q_off, refs_strings(r, r_off), diag, bo, nullptr);
}

extern "C" clh_band_plan* clh_band_plan_create_gap2(clh_ctx* ctx, int32_t n, const int8_t* q, const int64_t* q_off, const int8_t* r, const int64_t* r_off,
                                                    const int32_t* diag, const clh_band_opts* bo, const clh_gap2* gap2)
{
    if (!gap2) return clh_band_plan_create(ctx, n, q, q_off, r, r_off, diag, bo);
    return bd_create("clh_band_plan_create_gap2: ", ctx, n, q, q_off, refs_strings(r, r_off), diag, bo, gap2);
}

// K1gb on windows of the resident genome; gap2 may be null
extern "C" clh_band_plan* clh_band_plan_create_windows(clh_genome* genome, int32_t n, const int8_t* q, const int64_t* q_off, const int64_t* win_off,
                                                       const int32_t* win_len, const uint8_t* win_flags, const int32_t* diag, const clh_band_opts* bo,
                                                       const clh_gap2* gap2)
{
    const std::string me = "clh_band_plan_create_windows: ";
    if (!genome) { fail(CLH_E_ARG, me + "null genome"); return nullptr; }
    return bd_create(me, genome->ctx, n, q, q_off, refs_windows(genome, win_off, win_len, win_flags), diag, bo, gap2);
}

extern "C" int clh_band_plan_run(clh_band_plan* pl, void* stream_)
{
    if (!pl) return fail(CLH_E_ARG, "clh_band_plan_run: null argument");
    hipStream_t st;
    if (int rc = pairs_begin_run(pl, stream_, &st)) return rc;
    clh::Bd2Params p;
    p.go2 = pl->go2; p.ge2 = pl->ge2;
    p.qry = (const int8_t*)pl->d_q; p.ref = (const int8_t*)pl->d_r;
    p.pairs = (const clh::BdPair*)pl->d_pairs; p.npairs = pl->n;
    p.order = (const int32_t*)pl->d_order; p.norder = (int32_t)pl->order.size();
    p.mat = (const int8_t*)pl->d_mat; p.n_mat = pl->n_mat;
    p.go = pl->go; p.ge = pl->ge; p.mode = pl->mode;
    p.ws = (uint8_t*)pl->d_ws; p.ws_cap = pl->ws_bytes;
    p.rows = (int32_t*)pl->d_rows;
    p.cigar = (uint32_t*)pl->d_cig; p.cigar_cap = pl->cig_cap;
    // in stream order: a share's walk has read the workspace before the next share fills it
    auto run_shares = [&](auto launch, auto launch_walk) -> int {
        for (size_t s = 0; s < pl->shares.size(); ++s) {
            const auto& sh = pl->shares[s];
            const auto& cl = pl->share_classes[s];
            for (int c = 0; c < clh::kBdClasses; ++c) HIPCHK(launch(p, c, pl->want_cigar, cl.cfirst[c], cl.ccount[c], st));
            if (pl->want_cigar) HIPCHK(launch_walk(p, sh.first, sh.second, st));
        }
        return 0;
    };
    const int rc = pl->pieces == 2 ? run_shares(clh::launch_ssw_band2, clh::launch_ssw_band2_walk)
                                   : run_shares(clh::launch_ssw_band, clh::launch_ssw_band_walk);      // the one-piece launchers take the block's base
    return rc ? rc : pl->end_run();
}

// 1: the unbanded programme provably returns the same row and CIGAR (the argument is in the header and in DESIGN.md section 6).
// sh.gap(L) is the cost of one gap of L letters, one piece or two: all the proofs ask of it is that it does not decrease and that
// gap(a) + gap(b) >= gap(a + b), which go >= ge gives one piece and the admitted two-piece costs keep.
static int32_t bd_exact(int mode, int64_t m, int64_t n, int64_t lo, int64_t hi, int64_t score, int64_t splus, const PairsShape& sh)
{
    if (lo <= -m && hi >= n) return 1;
    if (mode == CLH_ENDS_PREFIX || mode == CLH_ENDS_EXTEND) {
        // the far end is free: an alignment that leaves the band need not come back, so one gap run and the M columns it leaves
        bool in = true;
        if (hi + 1 <= n) in = in && score > splus * std::min<int64_t>(m, n - hi - 1) - sh.gap(hi + 1);
        if (lo - 1 >= -m) in = in && score > splus * std::min<int64_t>(n, m + lo - 1) - sh.gap(1 - lo);
        return in ? 1 : 0;
    }
    if (mode != CLH_ENDS_GLOBAL) return 0;
    // the run that reaches diagonal hi + 1 (lo - 1) and the run that comes back to diagonal n - m: a global band holds n - m, so
    // both have at least one letter
    bool ok = true;
    if (hi + 1 <= n) ok = ok && score > splus * std::max<int64_t>(0, n - hi - 1) - sh.gap(hi + 1) - sh.gap(hi + 1 - (n - m));
    if (lo - 1 >= -m) ok = ok && score > splus * std::max<int64_t>(0, m + lo - 1) - sh.gap(1 - lo) - sh.gap(n - m - lo + 1);
    return ok ? 1 : 0;
}

extern "C" int clh_band_plan_fetch(clh_band_plan* pl, clh_band_row* rows, uint32_t* cigar, int64_t cigar_cap, int64_t* cigar_used)
{
    return pairs_fetch("band", pl, rows, cigar, cigar_cap, cigar_used, [pl](const clh::BdPair& p, clh_band_row& out) {
        // an admitted band of a pair with an empty side is the whole boundary, but for the row 0 of a semiglobal pair without a query
        // letter, whose first cell in the band is column lo
        if (pl->mode == CLH_ENDS_SEMIGLOBAL && p.m == 0) { out.ref_begin = p.lo; out.ref_end = p.lo - 1; }
        out.band_lo = p.lo; out.band_hi = p.hi; out.reserved = 0;
        out.exact = bd_exact(pl->mode, p.m, p.n, p.lo, p.hi, out.score, pl->splus, *pl);
    });
}

extern "C" int clh_band_plan_timing(clh_band_plan* pl, float* ms)
{
    if (!pl || !ms || !pl->ran) return fail(CLH_E_ARG, "clh_band_plan_timing: no run to time");
    return pl->elapsed(ms);
}

extern "C" int clh_band_plan_gather_timing(clh_band_plan* pl, float* ms, int64_t* letters)
{
    return pairs_gather_timing("clh_band_plan_gather_timing: ", pl, ms, letters);
}

extern "C" int clh_band_plan_info(clh_band_plan* pl, int64_t* out)
{
    if (!pl || !out) return fail(CLH_E_ARG, "clh_band_plan_info: null argument");
    for (int c = 0; c < clh::kBdClasses; ++c) { out[c] = clh::kBdCpl[c]; out[7 + c] = pl->nclass[c]; }
    out[3] = pl->max_width; out[4] = (int64_t)pl->shares.size(); out[5] = pl->ws_bytes; out[6] = pl->max_pair_ws;
    out[10] = pl->nempty; out[11] = pl->cig_cap;
    return 0;
}

extern "C" int clh_band_batch(clh_ctx* ctx, int32_t n, const int8_t* q, const int64_t* q_off, const int8_t* r, const int64_t* r_off, const int32_t* diag,
                              const clh_band_opts* opts, clh_band_row* rows, uint32_t* cigar, int64_t cigar_cap, int64_t* cigar_used)
{
    return pairs_batch(clh_band_plan_create(ctx, n, q, q_off, r, r_off, diag, opts), clh_band_plan_run, clh_band_plan_fetch, rows, cigar, cigar_cap, cigar_used);
}

extern "C" int clh_band_batch_gap2(clh_ctx* ctx, int32_t n, const int8_t* q, const int64_t* q_off, const int8_t* r, const int64_t* r_off, const int32_t* diag,
                                   const clh_band_opts* opts, const clh_gap2* gap2, clh_band_row* rows, uint32_t* cigar, int64_t cigar_cap, int64_t* cigar_used)
{
    return pairs_batch(clh_band_plan_create_gap2(ctx, n, q, q_off, r, r_off, diag, opts, gap2), clh_band_plan_run, clh_band_plan_fetch, rows, cigar, cigar_cap, cigar_used);
}

extern "C" void clh_encode_dna(const char* seq, int64_t len, int8_t* out)
{
    static int8_t lut[256];
    static bool init = false;
    if (!init) {
        memset(lut, 4, sizeof(lut));
        lut['A'] = lut['a'] = 0; lut['C'] = lut['c'] = 1; lut['G'] = lut['g'] = 2; lut['T'] = lut['t'] = 3; lut['N'] = lut['n'] = 4;
        init = true;
    }
    for (int64_t i = 0; i < len; ++i) out[i] = lut[(unsigned char)seq[i]];
}

// ------------------------------------------------------------------------------------------------------------
// the reference's six symbols (include/ssw_legacy.h)
// ------------------------------------------------------------------------------------------------------------
struct _profile {
    const int8_t* read;
    const int8_t* mat;
    int32_t readLen;
    int32_t n;
    int8_t score_size;
};

static clh_ctx* legacy_ctx()
{
    static std::mutex mu;
    static clh_ctx* ctx = nullptr;
    std::lock_guard<std::mutex> g(mu);
    if (!ctx) {
        const char* d = getenv("CIRI_LONG_DEVICE");
        ctx = clh_create(d ? atoi(d) : 0);
        if (!ctx) fprintf(stderr, "libclh: no usable GPU (%s); there is no CPU fallback.\n", clh_last_error());
    }
    return ctx;
}

extern "C" s_profile* ssw_init(const int8_t* read, const int32_t readLen, const int8_t* mat, const int32_t n, const int8_t score_size)
{
    s_profile* p = (s_profile*)calloc(1, sizeof(struct _profile));
    p->read = read; p->mat = mat; p->readLen = readLen; p->n = n; p->score_size = score_size;
    return p;
}

extern "C" void init_destroy(s_profile* p) { free(p); }

extern "C" s_align* ssw_align(const s_profile* prof, const int8_t* ref, int32_t refLen, const uint8_t weight_gapO,
                              const uint8_t weight_gapE, const uint8_t flag, const uint16_t filters, const int32_t filterd,
                              const int32_t maskLen)
{
    if (maskLen < 15)
        fprintf(stderr, "When maskLen < 15, the function ssw_align doesn't return 2nd best alignment information.\n");
    if (!(prof->score_size == 0 || prof->score_size == 1 || prof->score_size == 2)) {
        fprintf(stderr, "Please call the function ssw_init before ssw_align.\n");
        return NULL;
    }
    clh_ctx* ctx = legacy_ctx();
    if (!ctx) return NULL;
    clh_ssw_opts o;
    memset(&o, 0, sizeof(o));
    o.mat = prof->mat; o.n_mat = prof->n; o.gap_open = weight_gapO; o.gap_extend = weight_gapE; o.flag = flag;
    o.score_size = prof->score_size; o.filters = filters; o.filterd = filterd; o.want_score2 = 1; o.want_cigar = 1;
    const int64_t roff[2] = {0, prof->readLen}, foff[2] = {0, refLen};
    const int32_t ml = maskLen;
    clh_align_t a;
    std::vector<uint32_t> cig((size_t)2 * (size_t)std::max(prof->readLen, 1) + 8);
    int64_t used = 0;
    int rc = clh_ssw_batch(ctx, 1, prof->read, roff, ref, foff, &ml, &o, &a, cig.data(), (int64_t)cig.size(), &used);
    if (rc != 0) { fprintf(stderr, "libclh: ssw_align failed: %s\n", clh_last_error()); return NULL; }
    if (a.status & CLH_ST_NULL) {
        fprintf(stderr, "Please set 2 to the score_size parameter of the function ssw_init, otherwise the alignment results will be incorrect.\n");
        return NULL;
    }
    if (a.status & (CLH_ST_TRACE_ERR | CLH_ST_CIGAR_TRUNC)) { fprintf(stderr, "Trace back error.\n"); return NULL; }
    s_align* r = (s_align*)calloc(1, sizeof(s_align));
    r->score1 = a.score1; r->score2 = a.score2; r->ref_end1 = a.ref_end1; r->read_end1 = a.read_end1; r->ref_end2 = a.ref_end2;
    r->ref_begin1 = a.ref_begin1; r->read_begin1 = a.read_begin1;
    r->cigar = 0; r->cigarLen = 0;
    if (a.cigar_len > 0 && a.cigar_off >= 0) {
        r->cigar = (uint32_t*)malloc(sizeof(uint32_t) * (size_t)a.cigar_len);
        memcpy(r->cigar, cig.data() + a.cigar_off, sizeof(uint32_t) * (size_t)a.cigar_len);
        r->cigarLen = a.cigar_len;
    }
    return r;
}

extern "C" void align_destroy(s_align* a)
{
    if (!a) return;
    free(a->cigar);
    free(a);
}

extern "C" char cigar_int_to_op(uint32_t cigar_int)
{
    static const char map[] = {'M', 'I', 'D', 'N', 'S', 'H', 'P', '=', 'X'};
    const uint32_t c = cigar_int & 0xfU;
    return c >= sizeof(map) ? 'M' : map[c];
}

extern "C" uint32_t cigar_int_to_len(uint32_t cigar_int) { return cigar_int >> 4; }

// ------------------------------------------------------------------------------------------------------------
// cyclic consensus: find_consensus for a batch of reads (K2 + K3)
// ------------------------------------------------------------------------------------------------------------
struct clh_ccs_plan;
static clh_ccs_plan* ccs_plan_create(clh_ctx* ctx, int32_t n, const int64_t* read_off, int mcap_hint, bool wide_hint = false);
extern "C" clh_ccs_plan* clh_ccs_plan_create(clh_ctx* ctx, int32_t n, const int64_t* read_off) { return ccs_plan_create(ctx, n, read_off, 0); }

struct clh_ccs_plan : clh_owned {
    using clh_owned::clh_owned;
    int n = 0, lcap = 0, lmax = 0, n_long = 0, nslots = 0, nslots_big = 0;
    void *d_long = nullptr, *d_k2ws = nullptr, *d_busy = nullptr;
    struct K2Class { int begin, count, lcap; };
    std::vector<K2Class> k2_classes;
    int64_t total = 0;
    size_t slot_bytes = 0, slot_bytes_big = 0;      // second tier: a few slots sized for the worst case of the batch
    void *d_off = nullptr, *d_scan = nullptr, *d_res = nullptr, *d_segs = nullptr, *d_ccs = nullptr, *d_ws = nullptr, *d_ws_big = nullptr,
         *d_counter = nullptr, *d_order = nullptr, *d_wide = nullptr;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};   // K2 start, K2 stop = K3 start, K3 stop
};

extern "C" void clh_ccs_plan_destroy(clh_ccs_plan* pl) { delete pl; }

// scores of the consensus step of find_consensus: local alignment with the numbers of the reference's call
// (tests/test_poa.py:30), consensus over the nodes crossed by at least half of the copies (oracle/ccs_oracle.c)
static clh::PoaScores ccs_scores() { clh::PoaScores s; s.algorithm = 0; s.m = 10; s.n = -4; s.g = -8; s.e = -2; s.q = -24; s.c = -1; s.min_cov = -1; return s; }

static clh_ccs_plan* ccs_plan_create(clh_ctx* ctx, int32_t n, const int64_t* read_off, int mcap_hint, bool wide_hint)
{
    if (!ctx || n < 0 || !read_off) { fail(CLH_E_ARG, "clh_ccs_plan_create: null argument"); return nullptr; }
    if (hipSetDevice(ctx->device) != hipSuccess) { fail(CLH_E_HIP, "hipSetDevice failed"); return nullptr; }
    clh_ccs_plan* pl = new clh_ccs_plan(ctx);
    pl->n = n; pl->total = read_off[n];
    int lmax = 1;
    std::vector<int32_t> order(n), long_idx;
    for (int i = 0; i < n; ++i) {
        const int64_t L = read_off[i + 1] - read_off[i];
        if (L < 0 || L > (1 << 24)) { fail(CLH_E_UNSUPPORTED, "read longer than 16 M bases"); delete pl; return nullptr; }
        lmax = std::max(lmax, (int)L);
        if (L > clh::kK2LdsMax) long_idx.push_back(i);     // scanned out of an HBM workspace (ccs_scan_long_kernel)
        order[i] = i;
    }
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return read_off[x + 1] - read_off[x] > read_off[y + 1] - read_off[y]; });
    pl->lcap = (std::min(lmax, clh::kK2LdsMax) + 63) & ~63;
    {   // K2 launch classes over the length-sorted order: the LDS block of a launch is sized for its longest read
        static const int T[] = {1024, 1536, 2048, 3072, 4096, 6144, 8192, 12288, 16384};
        auto cls_of = [&](int64_t L) { for (int t : T) if (L <= t) return std::min(t, pl->lcap); return pl->lcap; };
        for (int k = 0; k < n;) {
            const int c = cls_of(std::min<int64_t>(read_off[order[k] + 1] - read_off[order[k]], clh::kK2LdsMax));
            int e = k;
            while (e < n && cls_of(std::min<int64_t>(read_off[order[e] + 1] - read_off[order[e]], clh::kK2LdsMax)) == c) ++e;
            pl->k2_classes.push_back({k, e - k, c});
            k = e;
        }
    }
    pl->lmax = lmax; pl->n_long = (int)long_idx.size();
    // Workspace.  The worst case of a read of L bases is a graph of L+8 nodes against copies of L/2 + L/16 bases (period
    // <= L/2, tolerance period/8), every row kept and with several
    // in-edges -- ~6 bytes per cell of that -- while the common case (period of a few hundred bases) needs a small
    // fraction.  So the first-tier slots (16 waves per CU x 256 CUs) share a budget, a wave whose read outgrows its slot
    // claims one of a few worst-case slots, and whatever found none free runs in a second launch over those.  Both budgets
    // follow the free memory of the device (HBM is 288 GB on an MI355X; nothing here assumes it).
    // (A copy above 2800 bases, or scores outside the 16-bit cells, runs the wide form of the pass: 6 bytes per cell instead of 4.)
    const int mcap_worst = mcap_hint > 0 ? mcap_hint + 1 : lmax / 2 + lmax / 16 + 8;
    const bool wide_worst = mcap_worst > 2801 || wide_hint || getenv("CLH_POA_FORCE_WIDE") != nullptr;
    const size_t need_worst = wide_worst ? clh::poa_slot_bytes_host_w(lmax + 8, mcap_worst) : clh::poa_slot_bytes_host(lmax + 8, mcap_worst);
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { fail(CLH_E_HIP, "hipMemGetInfo failed"); delete pl; return nullptr; }
    { std::lock_guard<std::mutex> g(ctx->mu); for (auto& kv : ctx->cache) free_b += kv.first; }      // parked blocks are ours to reuse
    int slots_max = 4096;                            // 16 waves per CU x 256 CUs
    if (const char* e = getenv("CLH_POA_SLOTS")) slots_max = std::max(64, atoi(e));      // tuning experiments
    pl->nslots = (int)std::max<long long>(1, std::min<long long>(slots_max, std::max(n, 1)));
    unsigned long long budget = std::min<unsigned long long>(40ull << 30, (unsigned long long)(free_b * 0.40));
    if (const char* e = getenv("CLH_POA_BUDGET_MB")) budget = std::max(1ull, strtoull(e, nullptr, 10)) << 20;     // tests: force the second tier
    pl->slot_bytes = std::min<size_t>(need_worst, (size_t)((budget / (unsigned long long)pl->nslots) & ~255ull));
    pl->slot_bytes = std::max<size_t>(pl->slot_bytes, 4096);
    if (pl->slot_bytes < need_worst) {
        // a FEW worst-case slots: rounds 2-5 took up to 1024 of them (64 GB); a batch of reads up to 4.5 kb then held 87 GB per plan, more than
        // the context parks between plans, and the file stage paid a 40 GB hipMalloc / hipFree per 32 MB of input (8.6 s for a 100 000-read
        // file whose kernels take 30 ms).  What finds no large slot free runs in the second launch over them, as before.
        const unsigned long long budget_big = std::min<unsigned long long>(12ull << 30, (unsigned long long)(free_b * 0.10));
        pl->slot_bytes_big = need_worst;
        if (const char* e = getenv("CLH_POA_BIG_BYTES")) pl->slot_bytes_big = std::max<size_t>(4096, std::min<size_t>(need_worst, strtoull(e, nullptr, 10)));   // tests: large slots too small (status 1)
        pl->nslots_big = (int)std::max<unsigned long long>(1, std::min<unsigned long long>(256, budget_big / pl->slot_bytes_big));
        pl->nslots_big = std::min(pl->nslots_big, std::max(n, 1));
        if (const char* e = getenv("CLH_POA_BIG_SLOTS")) pl->nslots_big = std::max(1, std::min(pl->nslots_big, atoi(e)));       // tests: make the large slots scarce
    }
    auto oom = [&] { fail(CLH_E_HIP, "out of device memory while building the consensus plan"); delete pl; return nullptr; };
    pl->d_off = pl->upload(read_off, sizeof(int64_t) * (size_t)(n + 1));
    pl->d_scan = pl->alloc(sizeof(clh::CcsScan) * (size_t)std::max(n, 1));
    pl->d_res = pl->alloc(sizeof(clh::CcsResult) * (size_t)std::max(n, 1));
    pl->d_segs = pl->alloc(sizeof(int32_t) * 2 * clh::CCS_SEG_CAP * (size_t)std::max(n, 1));
    pl->d_ccs = pl->alloc((size_t)std::max<int64_t>(pl->total, 1) + 64);
    pl->d_ws = pl->alloc(pl->slot_bytes * (size_t)pl->nslots);
    pl->d_counter = pl->alloc(256);
    pl->d_order = n > 0 ? pl->upload(order.data(), sizeof(int32_t) * (size_t)n) : pl->alloc(sizeof(int32_t));
    pl->d_wide = pl->alloc(sizeof(int32_t) * (size_t)std::max(n, 1));       // reads for the wide form of K3's pass
    if (!pl->d_off || !pl->d_scan || !pl->d_res || !pl->d_segs || !pl->d_ccs || !pl->d_ws || !pl->d_counter || !pl->d_order || !pl->d_wide) return oom();
    if (pl->nslots_big) {
        pl->d_ws_big = pl->alloc(pl->slot_bytes_big * (size_t)pl->nslots_big);
        pl->d_busy = pl->alloc(sizeof(int) * (size_t)pl->nslots_big);
        if (!pl->d_ws_big || !pl->d_busy || hipMemset(pl->d_busy, 0, sizeof(int) * (size_t)pl->nslots_big) != hipSuccess) return oom();
    }
    if (pl->n_long) {
        pl->d_long = pl->upload(long_idx.data(), sizeof(int32_t) * (size_t)pl->n_long);
        pl->d_k2ws = pl->alloc(clh::k2_long_slot_bytes(lmax) * (size_t)pl->n_long);
        if (!pl->d_long || !pl->d_k2ws) return oom();
    }
    (void)hipMemset(pl->d_segs, 0, sizeof(int32_t) * 2 * clh::CCS_SEG_CAP * (size_t)std::max(n, 1));   // entries beyond nseg read as 0
    return pl;
}

// the K3 launches of a plan: first tier over every read, second tier over what found no slot large enough
static int launch_poa_tiers(clh_ccs_plan* pl, clh::CcsParams& P, hipStream_t st)
{
    P.poa_ws = (uint8_t*)pl->d_ws; P.work_counter = (int*)pl->d_counter; P.stats = (int*)pl->d_counter + 2;
    P.wide_list = (int32_t*)pl->d_wide; P.wide_count = (int*)pl->d_counter + 32;
    P.work_order = (const int32_t*)pl->d_order;
    P.slot_bytes = pl->slot_bytes; P.n = pl->n; P.lcap = pl->lcap; P.tier = 0;
    if (pl->nslots_big) { P.big_ws = (uint8_t*)pl->d_ws_big; P.big_slot_bytes = pl->slot_bytes_big; P.big_busy = (int*)pl->d_busy; P.n_big = pl->nslots_big; }
    HIPCHK(clh::launch_poa(P, pl->nslots, st));
    if (pl->nslots_big) {       // the reads the first tier left with status 1
        clh::CcsParams Q = P;
        Q.poa_ws = (uint8_t*)pl->d_ws_big; Q.slot_bytes = pl->slot_bytes_big; Q.work_counter = (int*)pl->d_counter + 1; Q.tier = 1;
        HIPCHK(clh::launch_poa(Q, pl->nslots_big, st));
    }
    {   // what the packed kernel put on the wide list (copies above 2800 bases, scores outside the 16-bit cells, a cell at the floor of
        // the range): the 32-bit form, over worst-case slots; nothing on the list: the waves leave at once
        clh::CcsParams Q = P;
        Q.work_counter = (int*)pl->d_counter + 33; Q.tier = 2; Q.n_big = 0;
        int slots = pl->nslots;
        if (pl->nslots_big) { Q.poa_ws = (uint8_t*)pl->d_ws_big; Q.slot_bytes = pl->slot_bytes_big; slots = pl->nslots_big; }
        HIPCHK(clh::launch_poa_wide(Q, std::min(slots, 512), st));
    }
    return 0;
}

extern "C" int clh_ccs_run(clh_ccs_plan* pl, const void* d_reads, void* stream_)
{
    if (!pl || !d_reads) return fail(CLH_E_ARG, "clh_ccs_run: null argument");
    HIPCHK(hipSetDevice(pl->ctx->device));
    hipStream_t st = stream_ ? (hipStream_t)stream_ : pl->ctx->stream;
    if (pl->n == 0) { pl->ran = true; pl->last_stream = st; return 0; }
    clh::CcsParams P;
    memset(&P, 0, sizeof(P));
    P.reads = (const int8_t*)d_reads; P.read_off = (const int64_t*)pl->d_off; P.scan = (clh::CcsScan*)pl->d_scan;
    P.results = (clh::CcsResult*)pl->d_res; P.segs = (int32_t*)pl->d_segs; P.ccs = (int8_t*)pl->d_ccs;
    P.n = pl->n; P.lcap = pl->lcap;
    P.long_idx = (const int32_t*)pl->d_long; P.k2_ws = (uint8_t*)pl->d_k2ws; P.k2_slot = clh::k2_long_slot_bytes(pl->lmax);
    P.n_long = pl->n_long; P.k2_lmax = pl->lmax; P.k2_lds_max = clh::kK2LdsMax;
    P.sc = ccs_scores();
    if (getenv("CLH_POA_FORCE_WIDE")) P.sc.algorithm |= 0x200;      // tests: every read through the wide (32-bit) form of the pass
    if (!pl->ev[0]) for (auto& e : pl->ev) HIPCHK(pl->event(&e));
    HIPCHK(hipMemsetAsync(pl->d_counter, 0, 256, st));        // the two work counters and every statistic of the run
    const bool trace = getenv("CLH_TRACE") != nullptr;
    HIPCHK(hipEventRecord(pl->ev[0], st));
    P.work_order = (const int32_t*)pl->d_order;
    for (size_t k = 0; k < pl->k2_classes.size(); ++k) {
        P.k2_begin = pl->k2_classes[k].begin; P.lcap = pl->k2_classes[k].lcap;
        HIPCHK(clh::launch_ccs_scan(P, pl->k2_classes[k].count, k == 0, st));
    }
    P.lcap = pl->lcap;
    if (trace) { fprintf(stderr, "[clh] K2 launched (n=%d lcap=%d)\n", pl->n, pl->lcap); HIPCHK(hipStreamSynchronize(st)); fprintf(stderr, "[clh] K2 done\n"); }
    HIPCHK(hipEventRecord(pl->ev[1], st));
    // K3's work list: by read length (the plan's order; by estimated cost after K2, heaviest first, was measured slower -- LABNOTES)
    if (int rc = launch_poa_tiers(pl, P, st)) return rc;
    if (trace) { fprintf(stderr, "[clh] K3 launched (slots %d x %zu, big %d x %zu)\n", pl->nslots, pl->slot_bytes, pl->nslots_big, pl->slot_bytes_big); HIPCHK(hipStreamSynchronize(st)); fprintf(stderr, "[clh] K3 done\n"); }
    HIPCHK(hipEventRecord(pl->ev[2], st));
    pl->last_stream = st; pl->ran = true;
    return 0;
}

// durations of the last run's two launches in ms: ms[0] = K2 ccs_scan_kernel, ms[1] = K3 poa_consensus_kernel
extern "C" int clh_ccs_plan_timing(clh_ccs_plan* pl, float* ms)
{
    if (!pl || !pl->ran || !pl->ev[0] || !ms) return fail(CLH_E_ARG, "no timed run");
    HIPCHK(hipSetDevice(pl->ctx->device));
    HIPCHK(hipStreamSynchronize(pl->last_stream));
    HIPCHK(hipEventElapsedTime(&ms[0], pl->ev[0], pl->ev[1]));
    HIPCHK(hipEventElapsedTime(&ms[1], pl->ev[1], pl->ev[2]));
    return 0;
}

extern "C" int clh_ccs_fetch(clh_ccs_plan* pl, clh_ccs_t* out, int32_t* segs, int8_t* ccs)
{
    if (!pl || !out) return fail(CLH_E_ARG, "clh_ccs_fetch: null argument");
    if (!pl->ran) return fail(CLH_E_ARG, "clh_ccs_fetch before clh_ccs_run");
    HIPCHK(hipSetDevice(pl->ctx->device));
    HIPCHK(hipStreamSynchronize(pl->last_stream));
    if (pl->n == 0) return 0;
    static_assert(sizeof(clh_ccs_t) == sizeof(clh::CcsResult), "result layout");
    HIPCHK(hipMemcpy(out, pl->d_res, sizeof(clh::CcsResult) * (size_t)pl->n, hipMemcpyDeviceToHost));
    if (segs) HIPCHK(hipMemcpy(segs, pl->d_segs, sizeof(int32_t) * 2 * clh::CCS_SEG_CAP * (size_t)pl->n, hipMemcpyDeviceToHost));
    if (ccs && pl->total > 0) HIPCHK(hipMemcpy(ccs, pl->d_ccs, (size_t)pl->total, hipMemcpyDeviceToHost));
    return 0;
}

// how the workspace tiers of the plan were used by the last run: out = {first-tier slots, bytes per slot, large slots,
// bytes per large slot, reads that ran in a large slot claimed by a first-tier wave, reads run by the second launch}
extern "C" int clh_ccs_plan_info(clh_ccs_plan* pl, int64_t* out)
{
    if (!pl || !out) return fail(CLH_E_ARG, "clh_ccs_plan_info: null argument");
    out[0] = pl->nslots; out[1] = (int64_t)pl->slot_bytes; out[2] = pl->nslots_big; out[3] = (int64_t)pl->slot_bytes_big; out[4] = out[5] = 0;
    if (pl->ran && pl->n > 0) {
        HIPCHK(hipSetDevice(pl->ctx->device));
        HIPCHK(hipStreamSynchronize(pl->last_stream));
        int st[2] = {0, 0};
        HIPCHK(hipMemcpy(st, (int*)pl->d_counter + 2, sizeof(st), hipMemcpyDeviceToHost));
        out[4] = st[0]; out[5] = st[1];
    }
    return 0;
}

// statistics of the last run: out[16] = {DP cells, DP row steps, alignments run a second time with every cell stored, reads per status 1..7 (lost to a limit of the kernel: 1
// workspace, 2 graph limits, 3 output, 4 sequence above 2800 bases, 5 back-track guard, 6 16-bit range, 7 alignment without a
// base), 0...}
extern "C" int clh_ccs_plan_stats(clh_ccs_plan* pl, int64_t* out)
{
    if (!pl || !out) return fail(CLH_E_ARG, "clh_ccs_plan_stats: null argument");
    for (int k = 0; k < 16; ++k) out[k] = 0;
    if (pl->ran && pl->n > 0) {
        HIPCHK(hipSetDevice(pl->ctx->device));
        HIPCHK(hipStreamSynchronize(pl->last_stream));
        int st[64];
        HIPCHK(hipMemcpy(st, pl->d_counter, sizeof(st), hipMemcpyDeviceToHost));
        const int* s2 = st + 2;                                  // P.stats
        out[0] = (int64_t)((unsigned long long)(unsigned)s2[2] | ((unsigned long long)(unsigned)s2[3] << 32));
        out[1] = (int64_t)((unsigned long long)(unsigned)s2[4] | ((unsigned long long)(unsigned)s2[5] << 32));
        out[2] = s2[6];                                          // alignments whose walk left the band of stored cells (pass run again, everything stored)
        for (int k = 1; k <= 7; ++k) out[2 + k] = s2[8 + k];
    }
    return 0;
}

// device pointers of the last run's outputs, for callers that keep post-processing on the GPU: rows (clh_ccs_t[n]),
// segs (int32[n][2*65]) and the packed consensus codes (offsets = the read offsets of the plan)
extern "C" int clh_ccs_results_dev(const clh_ccs_plan* pl, const void** rows, const void** segs, const void** ccs)
{
    if (!pl) return fail(CLH_E_ARG, "clh_ccs_results_dev: null plan");
    if (rows) *rows = pl->d_res;
    if (segs) *segs = pl->d_segs;
    if (ccs) *ccs = pl->d_ccs;
    return 0;
}

extern "C" int clh_ccs_batch(clh_ctx* ctx, int32_t n, const int8_t* reads, const int64_t* read_off, clh_ccs_t* out, int32_t* segs, int8_t* ccs)
{
    if (!ctx || !reads || !read_off || !out) return fail(CLH_E_ARG, "clh_ccs_batch: null argument");
    static const bool trace = getenv("CLH_FILE_TRACE") != nullptr;
    auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t0 = trace ? now() : 0;
    clh_ccs_plan* pl = clh_ccs_plan_create(ctx, n, read_off);
    if (!pl) return g_code;
    const double t1 = trace ? now() : 0;
    int rc = 0;
    void* d_reads = pl->alloc((size_t)read_off[n] + 64);
    if (!d_reads) rc = fail(CLH_E_HIP, "out of device memory for the batch");
    if (!rc && read_off[n] > 0 && hipMemcpyAsync(d_reads, reads, (size_t)read_off[n], hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
        rc = fail(CLH_E_HIP, "H2D reads failed");
    if (!rc) rc = clh_ccs_run(pl, d_reads, nullptr);
    double t2 = 0, t3 = 0;
    if (trace) { t2 = now(); (void)hipStreamSynchronize(ctx->stream); t3 = now(); }
    if (!rc) rc = clh_ccs_fetch(pl, out, segs, ccs);
    const double t4 = trace ? now() : 0;
    delete pl;
    if (trace) fprintf(stderr, "[clh] ccs batch of %d reads: plan %.2f ms, H2D + launches %.2f, kernels (wait) %.2f, fetch %.2f, destroy %.2f\n", n,
                       (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t4 - t3) * 1e3, (now() - t4) * 1e3);
    return rc;
}

extern "C" int clh_poa_last_stats(clh_ctx* ctx, int64_t* out)
{
    if (!ctx || !out) return fail(CLH_E_ARG, "clh_poa_last_stats: null argument");
    for (int k = 0; k < 16; ++k) out[k] = ctx->last_poa_stats[k];
    return 0;
}

// spoa's AlignmentEngine::Create rules + what the kernel's 16-bit cells can hold
static int poa_check_opts(const clh_poa_opts* o, clh::PoaScores* s)
{
    clh_poa_opts d;
    d.algorithm = 0; d.m = 10; d.n = -4; d.g = -8; d.e = -2; d.q = -24; d.c = -1; d.min_coverage = 0;
    if (o) d = *o;
    if (d.algorithm < 0 || d.algorithm > 2) return fail(CLH_E_ARG, "poa: algorithm must be 0 (local), 1 (global) or 2 (overlap)");
    if (d.g > 0 || d.q > 0) return fail(CLH_E_ARG, "poa: gap opening penalty must be non-positive");
    if (d.e > 0 || d.c > 0) return fail(CLH_E_ARG, "poa: gap extension penalty must be non-positive");
    if (d.g >= d.e) return fail(CLH_E_UNSUPPORTED, "poa: linear gap cost (g >= e) is not built into the kernel");
    if (d.g <= d.q || d.e >= d.c) { d.q = d.g; d.c = d.e; }          // affine: one piece
    if (d.m < 1 || d.n > d.m) return fail(CLH_E_UNSUPPORTED, "poa: match score must be positive and not below the mismatch score");
    if (d.e - d.g > 6 || d.c - d.q > 30) return fail(CLH_E_UNSUPPORTED, "poa: e - g <= 6 and c - q <= 30 required (vertical gap states are kept as small differences)");
    if (d.m > 100000 || d.n < -100000 || d.g < -100000 || d.q < -100000) return fail(CLH_E_UNSUPPORTED, "poa: scores beyond +-100000");
    // scores that leave the 16-bit cells of the packed pass (match above 11, a mismatch or gap extension that drives 2800 bases below
    // -30000, the row scans' frames H - j*e, H - j*c over the 512 columns of a pass) run the wide form of the pass for every sequence
    bool wide = d.m > 11 || d.n < -100;
    wide = wide || std::max(d.g + 2799 * d.e, d.q + 2799 * d.c) < -30000;
    wide = wide || d.m * 2800 + 512 * std::max(-d.e, -d.c) > 32767;
    if (getenv("CLH_POA_FORCE_WIDE")) wide = true;
    if (d.min_coverage < 0) return fail(CLH_E_ARG, "poa: min_coverage must be >= 0");
    s->algorithm = d.algorithm | (wide ? 0x200 : 0); s->m = d.m; s->n = d.n; s->g = d.g; s->e = d.e; s->q = d.q; s->c = d.c; s->min_cov = d.min_coverage;
    return 0;
}

// consensus of explicit groups of sequences (the spoa.poa call shape): group k = sequences [group_off[k], group_off[k+1])
extern "C" int clh_poa_batch(clh_ctx* ctx, int32_t ngroups, const int8_t* seqs, const int64_t* seq_off, const int64_t* group_off,
                             const clh_poa_opts* opts, int32_t* out_len, int8_t* out_ccs, int32_t* msa_col, int32_t* msa_ncols, int32_t* aln_score)
{
    if (!ctx || ngroups < 0 || !seqs || !seq_off || !group_off || !out_len || !out_ccs) return fail(CLH_E_ARG, "clh_poa_batch: null argument");
    clh::PoaScores sc;
    if (int rc = poa_check_opts(opts, &sc)) return rc;
    std::vector<int64_t> roff((size_t)ngroups + 1), xoff((size_t)ngroups + 1);
    std::vector<int32_t> xcuts;
    for (int k = 0; k < ngroups; ++k) {
        const int64_t s0 = group_off[k], s1 = group_off[k + 1];
        if (s1 - s0 < 1) return fail(CLH_E_ARG, "a consensus group must hold at least one sequence");
        if (seq_off[s1] - seq_off[s0] > (1 << 24)) return fail(CLH_E_UNSUPPORTED, "a consensus group above 16 M bases");
        roff[k] = seq_off[s0];
        xoff[k] = (int64_t)xcuts.size();
        for (int64_t i = s0 + 1; i < s1; ++i) xcuts.push_back((int32_t)(seq_off[i] - seq_off[s0]));
    }
    xoff[ngroups] = (int64_t)xcuts.size();
    roff[ngroups] = ngroups ? seq_off[group_off[ngroups]] : 0;
    // groups must tile the packed array contiguously
    for (int k = 0; k + 1 < ngroups; ++k) if (seq_off[group_off[k + 1]] != roff[k + 1]) return fail(CLH_E_ARG, "groups must be contiguous");
    if (ngroups == 0) return 0;
    int mcap = 1;
    for (int64_t i = 0; i < group_off[ngroups]; ++i) mcap = std::max<int>(mcap, (int)(seq_off[i + 1] - seq_off[i]));
    // (global and overlap alignments can sink below the 16-bit cells with any scores: their large slots are sized for the wide form, so that
    // a group the packed kernel hands over finds room there)
    clh_ccs_plan* pl = ccs_plan_create(ctx, ngroups, roff.data(), mcap, (sc.algorithm & 0x200) != 0 || (sc.algorithm & 0xff) != 0);
    if (!pl) return g_code;
    int rc = 0;
    const size_t total = (size_t)roff[ngroups];
    void* d_reads = pl->alloc(total + 64);
    void* d_xcuts = pl->alloc(sizeof(int32_t) * (xcuts.size() + 1));
    void* d_xoff = pl->alloc(sizeof(int64_t) * (size_t)(ngroups + 1));
    void* d_col = msa_col ? pl->alloc(sizeof(int32_t) * (total + 1)) : nullptr;
    void* d_ncols = msa_col ? pl->alloc(sizeof(int32_t) * (size_t)ngroups) : nullptr;
    void* d_score = aln_score ? pl->alloc(sizeof(int32_t) * clh::CCS_SEG_CAP * (size_t)ngroups) : nullptr;
    hipStream_t st = ctx->stream;
    if (!d_reads || !d_xcuts || !d_xoff || (msa_col && (!d_col || !d_ncols)) || (aln_score && !d_score)) rc = fail(CLH_E_HIP, "out of device memory");
    if (!rc && hipMemcpyAsync(d_reads, seqs, total, hipMemcpyHostToDevice, st) != hipSuccess) rc = fail(CLH_E_HIP, "H2D failed");
    if (!rc && !xcuts.empty() && hipMemcpyAsync(d_xcuts, xcuts.data(), sizeof(int32_t) * xcuts.size(), hipMemcpyHostToDevice, st) != hipSuccess) rc = fail(CLH_E_HIP, "H2D failed");
    if (!rc && hipMemcpyAsync(d_xoff, xoff.data(), sizeof(int64_t) * (size_t)(ngroups + 1), hipMemcpyHostToDevice, st) != hipSuccess) rc = fail(CLH_E_HIP, "H2D failed");
    if (!rc && aln_score && hipMemsetAsync(d_score, 0, sizeof(int32_t) * clh::CCS_SEG_CAP * (size_t)ngroups, st) != hipSuccess) rc = fail(CLH_E_HIP, "memset failed");
    if (!rc) {
        clh::CcsParams P;
        memset(&P, 0, sizeof(P));
        P.reads = (const int8_t*)d_reads; P.read_off = (const int64_t*)pl->d_off; P.scan = (clh::CcsScan*)pl->d_scan;
        P.results = (clh::CcsResult*)pl->d_res; P.segs = (int32_t*)pl->d_segs; P.ccs = (int8_t*)pl->d_ccs;
        P.sc = sc; P.xcuts = (const int32_t*)d_xcuts; P.xcut_off = (const int64_t*)d_xoff;
        P.msa_col = (int32_t*)d_col; P.msa_ncols = (int32_t*)d_ncols; P.aln_score = (int32_t*)d_score;
        if (hipMemsetAsync(pl->d_counter, 0, 256, st) != hipSuccess) rc = fail(CLH_E_HIP, "memset failed");
        if (!rc) rc = launch_poa_tiers(pl, P, st);
        pl->ran = true; pl->last_stream = st;
    }
    if (!rc) {
        std::vector<clh_ccs_t> res((size_t)ngroups);
        rc = clh_ccs_fetch(pl, res.data(), nullptr, out_ccs);
        for (int k = 0; k < ngroups && !rc; ++k) out_len[k] = res[k].nseg > 0 && res[k].status == 0 ? res[k].ccs_len : -(1 + res[k].status);
        if (!rc && msa_col && (hipMemcpy(msa_col, d_col, sizeof(int32_t) * total, hipMemcpyDeviceToHost) != hipSuccess ||
                               (msa_ncols && hipMemcpy(msa_ncols, d_ncols, sizeof(int32_t) * (size_t)ngroups, hipMemcpyDeviceToHost) != hipSuccess)))
            rc = fail(CLH_E_HIP, "D2H failed");
        if (!rc && aln_score && hipMemcpy(aln_score, d_score, sizeof(int32_t) * clh::CCS_SEG_CAP * (size_t)ngroups, hipMemcpyDeviceToHost) != hipSuccess)
            rc = fail(CLH_E_HIP, "D2H failed");
    } else (void)hipStreamSynchronize(st);
    if (!rc) (void)clh_ccs_plan_stats(pl, ctx->last_poa_stats);
    delete pl;
    return rc;
}

// ---------------------------------------------------------------------------------------------------------------
// K7: minimizer index of the resident genome, seeds and chains (seed.hip, seed_sort.hip; definitions in seed_device.h)
// ---------------------------------------------------------------------------------------------------------------
#include "seed_device.h"

// device blocks of one call: given back, after the stream has drained, when the call returns
struct SdBlocks {
    clh_ctx* ctx;
    std::vector<void*> v;
    size_t refused = 0;                                 // bytes of the first allocation the device refused
    explicit SdBlocks(clh_ctx* c) : ctx(c) {}
    SdBlocks(const SdBlocks&) = delete;
    ~SdBlocks() { (void)hipStreamSynchronize(ctx->stream); for (void* p : v) ctx->release(p); }
    template <class T> T* get(size_t count)
    {
        void* p = ctx->alloc(sizeof(T) * (count ? count : 1));
        if (p) v.push_back(p); else if (!refused) refused = sizeof(T) * count;
        return (T*)p;
    }
    template <class T> T* put(const std::vector<T>& h)
    {
        T* p = get<T>(h.size());
        if (p && !h.empty() && hipMemcpyAsync(p, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice, ctx->stream) != hipSuccess) return nullptr;
        return p;
    }
};
static int sd_refused(const std::string& me, const SdBlocks& B)
{
    return fail(CLH_E_CAPACITY, me + "the device refused an allocation" + (B.refused ? " of " + std::to_string(B.refused) + " bytes" : std::string()));
}
static int sd_bits(uint64_t v) { int b = 1; while (v >>= 1) ++b; return b; }

struct clh_seed_index : clh_owned {
    using clh_owned::clh_owned;
    clh_genome* genome = nullptr;
    int k = 0, w = 0, max_occ = 0, last_shares = 0;
    std::vector<int64_t> c_off, c_len;
    int64_t *d_coff = nullptr, *d_clen = nullptr;
    uint64_t *d_keys = nullptr, *d_vals = nullptr;
    int64_t n = 0, distinct = 0, over = 0, bytes = 0;
    float ms[5] = {0, 0, 0, 0, 0};
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    std::vector<uint64_t> h_mkeys, h_mvals, h_k1, h_k2;          // what the last minimizers / seeds call left for its fetch
    hipEvent_t cev[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};      // around the kernels of clh_seed_circle_batch
    std::vector<int64_t> h_table;                                // what the last circles call left for clh_seed_circle_table_fetch
};

extern "C" void clh_seed_index_destroy(clh_seed_index* x) { delete x; }

// the sketch of nseq sequences of d_codes: entries in (sequence, position) order, in blocks of B
// The host tables that are uploaded asynchronously live here too: an SdEntries (and every other host buffer of an asynchronous copy) is
// declared BEFORE the call's SdBlocks, whose destructor drains the stream, so that on every return, early ones included, no copy in
// flight outlives its host side.
struct SdEntries {
    uint64_t *keys = nullptr, *vals = nullptr; int32_t* seq_of = nullptr; int64_t n = 0; int64_t *d_item_off = nullptr, *d_seq_item0 = nullptr;
    std::vector<int64_t> h_item0; std::vector<int32_t> h_item_seq;
};
static int sd_sketch(const std::string& me, clh_seed_index* x, SdBlocks& B, const uint8_t* d_codes, int64_t codes_len, const std::vector<int64_t>& off,
                     const std::vector<int64_t>& len, bool global_pos, bool want_seq, SdEntries* o)
{
    hipStream_t st = x->ctx->stream;
    const int32_t nseq = (int32_t)off.size();
    std::vector<int64_t>& item0 = o->h_item0;
    std::vector<int32_t>& item_seq = o->h_item_seq;
    item0.assign((size_t)nseq + 1, 0); item_seq.clear();
    for (int32_t s = 0; s < nseq; ++s) {
        const int64_t P = len[s] - x->k + 1, items = P > 0 ? (P + clh::kSdItem - 1) / clh::kSdItem : 0;
        item0[s + 1] = item0[s] + items;
        item_seq.insert(item_seq.end(), (size_t)items, s);
    }
    const int64_t nitems = item0[nseq];
    clh::SdSketch S;
    S.codes = d_codes; S.codes_len = codes_len; S.nseq = nseq; S.nitems = nitems; S.k = x->k; S.w = x->w; S.global_pos = global_pos ? 1 : 0;
    S.off = B.put(off); S.len = B.put(len); S.item_seq = B.put(item_seq); S.seq_item0 = o->d_seq_item0 = B.put(item0);
    int32_t* d_count = B.get<int32_t>((size_t)nitems + 1);
    o->d_item_off = B.get<int64_t>((size_t)nitems + 1);
    const size_t tb = clh::seed_scan_temp_bytes(nitems + 1);
    void* d_temp = B.get<uint8_t>(tb);
    if (!S.off || !S.len || !S.item_seq || !S.seq_item0 || !d_count || !o->d_item_off || !d_temp) return sd_refused(me, B);
    HIPCHK(hipMemsetAsync(d_count, 0, sizeof(int32_t) * ((size_t)nitems + 1), st));
    HIPCHK(clh::launch_seed_sketch_count(S, d_count, st));
    HIPCHK(clh::seed_scan_counts(d_temp, tb, d_count, o->d_item_off, nitems + 1, st));
    HIPCHK(hipMemcpyAsync(&o->n, o->d_item_off + nitems, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (o->n < 0) return fail(CLH_E_HIP, me + "the count pass left a negative total");
    o->keys = B.get<uint64_t>((size_t)o->n); o->vals = B.get<uint64_t>((size_t)o->n);
    if (want_seq) o->seq_of = B.get<int32_t>((size_t)o->n);
    if (!o->keys || !o->vals || (want_seq && !o->seq_of)) return sd_refused(me, B);
    HIPCHK(clh::launch_seed_sketch_fill(S, o->d_item_off, o->keys, o->vals, o->seq_of, o->n, st));
    return 0;
}

static int sd_build(const std::string& me, clh_seed_index* x)
{
    clh_ctx* ctx = x->ctx;
    hipStream_t st = ctx->stream;
    SdEntries E;                                        // before B: see SdEntries
    SdBlocks B(ctx);
    HIPCHK(hipEventRecord(x->ev[0], st));
    if (int rc = sd_sketch(me, x, B, (const uint8_t*)x->genome->d_codes, x->genome->len, x->c_off, x->c_len, true, false, &E)) return rc;
    HIPCHK(hipEventRecord(x->ev[1], st));
    x->n = E.n;
    x->d_keys = (uint64_t*)x->alloc(sizeof(uint64_t) * (size_t)(E.n ? E.n : 1));
    x->d_vals = (uint64_t*)x->alloc(sizeof(uint64_t) * (size_t)(E.n ? E.n : 1));
    const size_t tb = clh::seed_sort_temp_bytes(E.n);
    void* d_temp = B.get<uint8_t>(tb);
    unsigned long long* d_stats = B.get<unsigned long long>(2);
    if (!x->d_keys || !x->d_vals || !d_temp || !d_stats)
        return fail(CLH_E_CAPACITY, me + "the device refused the " + std::to_string(16 * (size_t)E.n + tb) + " bytes of the sorted index of " + std::to_string(E.n) + " entries");
    HIPCHK(clh::seed_sort_pairs(d_temp, tb, E.keys, x->d_keys, E.vals, x->d_vals, E.n, 2 * x->k, st));
    HIPCHK(hipEventRecord(x->ev[2], st));
    HIPCHK(hipMemsetAsync(d_stats, 0, 16, st));
    HIPCHK(clh::launch_seed_index_stats(x->d_keys, E.n, x->max_occ, d_stats, st));
    unsigned long long stats[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(stats, d_stats, 16, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipEventElapsedTime(&x->ms[0], x->ev[0], x->ev[1]));
    HIPCHK(hipEventElapsedTime(&x->ms[1], x->ev[1], x->ev[2]));
    x->distinct = (int64_t)stats[0]; x->over = (int64_t)stats[1];
    x->bytes = 16 * (E.n ? E.n : 1) + 16 * (int64_t)x->c_off.size();
    return 0;
}

extern "C" clh_seed_index* clh_seed_index_create(clh_genome* g, int32_t k, int32_t w, int32_t n_contigs, const int64_t* contig_off, const int64_t* contig_len,
                                                 int32_t max_occ)
{
    const std::string me = "clh_seed_index_create: ";
    if (!g || n_contigs < 0 || (n_contigs > 0 && (!contig_off || !contig_len))) { fail(CLH_E_ARG, me + "null argument"); return nullptr; }
    if (k < clh::kSdKMin || k > clh::kSdKMax) { fail(CLH_E_ARG, me + "k must be 4..28, got " + std::to_string(k)); return nullptr; }
    if (w < clh::kSdWMin || w > clh::kSdWMax) { fail(CLH_E_ARG, me + "w must be 1..64, got " + std::to_string(w)); return nullptr; }
    if (max_occ < 1) { fail(CLH_E_ARG, me + "max_occ must be at least 1"); return nullptr; }
    if (g->len >= ((int64_t)1 << 39)) { fail(CLH_E_CAPACITY, me + "a genome of 2^39 bases or more"); return nullptr; }
    for (int32_t c = 0; c < n_contigs; ++c)
        if (contig_off[c] < 0 || contig_len[c] < 0 || contig_off[c] + contig_len[c] > g->len || (c > 0 && contig_off[c] < contig_off[c - 1] + contig_len[c - 1])) {
            fail(CLH_E_ARG, me + "contig " + std::to_string(c) + " lies outside the genome or before the end of the contig in front of it"); return nullptr;
        }
    if (hipSetDevice(g->ctx->device) != hipSuccess) { fail(CLH_E_HIP, "hipSetDevice failed"); return nullptr; }
    clh_seed_index* x = new clh_seed_index(g->ctx);
    x->genome = g; x->k = k; x->w = w; x->max_occ = max_occ;
    x->c_off.assign(contig_off, contig_off + n_contigs); x->c_len.assign(contig_len, contig_len + n_contigs);
    bool ok = true;
    for (auto& e : x->ev) ok = ok && x->event(&e) == hipSuccess;
    for (auto& e : x->cev) ok = ok && x->event(&e) == hipSuccess;
    x->d_coff = (int64_t*)x->upload(x->c_off.data(), sizeof(int64_t) * (size_t)n_contigs);
    x->d_clen = (int64_t*)x->upload(x->c_len.data(), sizeof(int64_t) * (size_t)n_contigs);
    if (!ok || !x->d_coff || !x->d_clen) { fail(CLH_E_HIP, me + "out of device memory"); delete x; return nullptr; }
    if (sd_build(me, x)) { (void)hipStreamSynchronize(g->ctx->stream); delete x; return nullptr; }
    return x;
}

extern "C" int clh_seed_index_info(clh_seed_index* x, int64_t* out)
{
    if (!x || !out) return fail(CLH_E_ARG, "clh_seed_index_info: null argument");
    const int64_t v[12] = {x->n, x->distinct, x->over, x->bytes, x->k, x->w, x->max_occ, x->last_shares, clh::kSdRound, clh::kSdItem, clh::kSdItemsPerBlock, 0};
    for (int i = 0; i < 12; ++i) out[i] = v[i];
    return 0;
}

extern "C" int clh_seed_index_timing(clh_seed_index* x, float* ms)
{
    if (!x || !ms) return fail(CLH_E_ARG, "clh_seed_index_timing: null argument");
    for (int i = 0; i < 5; ++i) ms[i] = x->ms[i];
    return 0;
}

extern "C" int clh_seed_index_dump(clh_seed_index* x, int64_t first, int64_t count, uint64_t* keys, int64_t* pos, uint8_t* strand)
{
    if (!x || count < 0 || (count > 0 && (!keys || !pos || !strand))) return fail(CLH_E_ARG, "clh_seed_index_dump: null argument");
    if (first < 0 || first + count > x->n) return fail(CLH_E_ARG, "clh_seed_index_dump: the range leaves the " + std::to_string(x->n) + " entries");
    if (count == 0) return 0;
    HIPCHK(hipSetDevice(x->ctx->device));
    std::vector<uint64_t> v((size_t)count);
    HIPCHK(hipMemcpy(keys, x->d_keys + first, sizeof(uint64_t) * (size_t)count, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(v.data(), x->d_vals + first, sizeof(uint64_t) * (size_t)count, hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < count; ++i) { pos[i] = (int64_t)(v[i] >> 1); strand[i] = (uint8_t)(v[i] & 1); }
    return 0;
}

// the reads of a call on the device and their sketch
struct SdReads { std::vector<int64_t> off, len; uint8_t* d_codes = nullptr; int64_t total = 0; SdEntries E; };
static int sd_reads(const std::string& me, clh_seed_index* x, SdBlocks& B, int32_t n, const int8_t* reads, const int64_t* read_off, SdReads* R)
{
    if (!x || n < 0 || !read_off) return fail(CLH_E_ARG, me + "null argument");
    if (read_off[0] < 0) return fail(CLH_E_ARG, me + "offsets must ascend from 0 or above");
    R->off.assign(read_off, read_off + n); R->len.resize((size_t)n);
    for (int32_t r = 0; r < n; ++r) {
        const int64_t L = read_off[r + 1] - read_off[r];
        if (L < 0) return fail(CLH_E_ARG, me + "offsets must ascend");
        if (L >= ((int64_t)1 << clh::kSdYBits)) return fail(CLH_E_ARG, me + "read " + std::to_string(r) + " has 2^24 letters or more");
        R->len[r] = L;
    }
    R->total = read_off[n];
    if (R->total > 0 && !reads) return fail(CLH_E_ARG, me + "null argument");
    for (int32_t r = 0; r < n; ++r)
        for (int64_t i = read_off[r]; i < read_off[r + 1]; ++i)
            if (reads[i] < 0 || reads[i] > 4) return fail(CLH_E_ARG, me + "read " + std::to_string(r) + " holds a code outside 0..4");
    HIPCHK(hipSetDevice(x->ctx->device));
    R->d_codes = B.get<uint8_t>((size_t)R->total);
    if (!R->d_codes) return sd_refused(me, B);
    if (R->total > 0) HIPCHK(hipMemcpyAsync(R->d_codes, reads, (size_t)R->total, hipMemcpyHostToDevice, x->ctx->stream));
    HIPCHK(hipEventRecord(x->ev[0], x->ctx->stream));
    return sd_sketch(me, x, B, R->d_codes, R->total, R->off, R->len, false, true, &R->E);
}

extern "C" int clh_seed_minimizers(clh_seed_index* x, int32_t n, const int8_t* seqs, const int64_t* seq_off, int64_t* min_off)
{
    const std::string me = "clh_seed_minimizers: ";
    if (!x || !min_off) return fail(CLH_E_ARG, me + "null argument");
    SdReads R;                                          // before B: see SdEntries
    std::vector<int64_t> item0, item_off;
    SdBlocks B(x->ctx);
    if (int rc = sd_reads(me, x, B, n, seqs, seq_off, &R)) return rc;
    hipStream_t st = x->ctx->stream;
    HIPCHK(hipEventRecord(x->ev[1], st));
    // min_off[r] = item_off[seq_item0[r]]: both tables come back, the host does the look-up
    item0.resize((size_t)n + 1);
    HIPCHK(hipMemcpyAsync(item0.data(), R.E.d_seq_item0, sizeof(int64_t) * ((size_t)n + 1), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    item_off.resize((size_t)item0[n] + 1);
    HIPCHK(hipMemcpyAsync(item_off.data(), R.E.d_item_off, sizeof(int64_t) * item_off.size(), hipMemcpyDeviceToHost, st));
    x->h_mkeys.assign((size_t)R.E.n, 0); x->h_mvals.assign((size_t)R.E.n, 0);
    if (R.E.n > 0) {
        HIPCHK(hipMemcpyAsync(x->h_mkeys.data(), R.E.keys, sizeof(uint64_t) * (size_t)R.E.n, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(x->h_mvals.data(), R.E.vals, sizeof(uint64_t) * (size_t)R.E.n, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipEventElapsedTime(&x->ms[2], x->ev[0], x->ev[1]));
    for (int32_t r = 0; r <= n; ++r) min_off[r] = item_off[(size_t)item0[r]];
    return 0;
}

extern "C" int clh_seed_minimizers_fetch(clh_seed_index* x, int64_t cap, int64_t* pos, uint64_t* keys, uint8_t* strand)
{
    if (!x) return fail(CLH_E_ARG, "clh_seed_minimizers_fetch: null argument");
    const int64_t m = (int64_t)x->h_mkeys.size();
    if (cap < m) return fail(CLH_E_CAPACITY, "clh_seed_minimizers_fetch: cap too small");
    if (m > 0 && (!pos || !keys || !strand)) return fail(CLH_E_ARG, "clh_seed_minimizers_fetch: null argument");
    for (int64_t i = 0; i < m; ++i) { keys[i] = x->h_mkeys[i]; pos[i] = (int64_t)(x->h_mvals[i] >> 1); strand[i] = (uint8_t)(x->h_mvals[i] & 1); }
    return 0;
}

static clh::LkParams lk_params(const clh_link_opts* l)
{
    return clh::LkParams{l->max_query_gap, l->max_overlap, l->max_skew, l->max_intron, l->max_circle, l->intron_cost, l->backsplice_cost};
}
static int lk_opts_check(const std::string& me, const clh_link_opts* l)
{
    if (l->max_query_gap < 0 || l->max_overlap < 0 || l->max_skew < 0 || l->max_intron < 0 || l->max_circle < 0 || l->intron_cost < 0 || l->backsplice_cost < 0)
        return fail(CLH_E_ARG, me + "no link parameter may be negative");
    if (l->max_skew > l->max_intron) return fail(CLH_E_ARG, me + "max_skew must not be above max_intron");
    if (l->intron_cost >= clh::kLkLimit || l->backsplice_cost >= clh::kLkLimit) return fail(CLH_E_ARG, me + "intron_cost and backsplice_cost must be below 2^40");
    return 0;
}
// what the link kernel left for segments [s0, s0 + nseg), whose chain counts are in seg: every header and every row of a chain written
static int lk_validate(const std::string& me, int64_t s0, int64_t nseg, int32_t max_chains, const int64_t* seg, const int64_t* lseg, const int64_t* lrows)
{
    for (int64_t s = 0; s < nseg; ++s) {
        const int64_t* h = lseg + clh::kLkSeg * s;
        const int64_t nc = seg[clh::kChSeg * s];
        if (h[0] == clh::kChUnwritten || h[0] != nc || h[1] < 0 || h[1] > nc || (nc > 0 && h[1] == 0) || h[3] != 0)
            return fail(CLH_E_HIP, me + "the link kernel left segment " + std::to_string(s0 + s) +
                                       (h[0] == clh::kChUnwritten ? " unwritten" : " with " + std::to_string(h[0]) + " chains of " + std::to_string(nc) + ", status " + std::to_string(h[3])));
        for (int64_t c = 0; c < nc; ++c) {
            const int64_t* r = lrows + ((s * max_chains) + c) * clh::kLkRow;
            if (r[7] != 0 || r[0] < 0 || r[0] >= nc || r[2] < -1 || r[2] >= nc || r[4] < 0 || r[4] >= h[1] || r[5] < 0 || r[5] >= nc)
                return fail(CLH_E_HIP, me + "the link kernel left a row of segment " + std::to_string(s0 + s) + (r[7] != 0 ? " unwritten" : " out of range"));
        }
    }
    return 0;
}

// what K7j admits of its scoring: clh_seed_junction_batch and clh_seed_circle_batch refuse the same
static int jx_opts_check(const std::string& me, const clh_junction_opts* o, const clh_splice* sp)
{
    if (o->max_span < 1 || o->max_span > clh::kJxMaxSpan) return fail(CLH_E_ARG, me + "max_span must be 1.." + std::to_string(clh::kJxMaxSpan));
    if (o->slack < 0 || o->slack > clh::kJxMaxSlack) return fail(CLH_E_ARG, me + "slack must be 0.." + std::to_string(clh::kJxMaxSlack));
    int64_t dmax = sp->other, amax = sp->other;
    bool neg = o->match < 0 || o->mismatch < 0 || o->gap_open < 0 || o->gap_extend < 0 || sp->intron_open < 0 || sp->other < 0;
    for (int k = 0; k < 16; ++k) {
        neg = neg || sp->donor[k] < 0 || sp->acceptor[k] < 0;
        dmax = std::max<int64_t>(dmax, sp->donor[k]); amax = std::max<int64_t>(amax, sp->acceptor[k]);
    }
    if (neg) return fail(CLH_E_ARG, me + "match, mismatch, the gap costs, intron_open, the donor and acceptor costs and `other` must not be negative");
    if (o->gap_open < o->gap_extend) return fail(CLH_E_UNSUPPORTED, me + "gap_open < gap_extend is not built");
    const int64_t cmax = std::max<int64_t>(std::max(o->match, o->mismatch), std::max(o->gap_open, o->gap_extend));
    if ((2 * (int64_t)o->max_span + o->slack) * cmax + sp->intron_open + dmax + amax >= clh::kJxBound)
        return fail(CLH_E_ARG, me + "(2 max_span + slack) max(match, mismatch, gap_open, gap_extend) + intron_open + dmax + amax must stay below 2^20: a side score "
                                    "less a site cost and a column index share one 32-bit key");
    return 0;
}

// ---- K7c: what clh_seed_circle_batch adds to sd_seeds (seed_circle.hip) ------------------------------------------------------------
// Declared by the caller BEFORE the call, as an SdEntries is: its host tables are uploaded asynchronously and outlive sd_seeds' SdBlocks.
struct SdCircle {
    const clh_junction_opts* jo = nullptr; const clh_splice* sp = nullptr;
    int64_t min_path_score = 0;
    int64_t* circle_out = nullptr; int64_t* cor_out = nullptr; int64_t* n_circles = nullptr;
    std::vector<int64_t> h_roff;
    std::vector<int32_t> site;
    unsigned long long h_count[clh::kJxClasses] = {0, 0, 0, 0};
    int64_t h_total = 0;
    float ms[3] = {0, 0, 0};
    clh::CcLaunch L; clh::JxLaunch J;
    int64_t* d_jout = nullptr;
    size_t slots_max = 0;                               // task slots of the largest share
};

// the buffers of the largest share and of the whole batch's circle rows
static int cc_prepare(const std::string& me, clh_seed_index* x, SdBlocks& B, const uint8_t* d_reads, int32_t n, int32_t reads_max, int32_t max_chains, SdCircle* cc)
{
    hipStream_t st = x->ctx->stream;
    memset(&cc->L, 0, sizeof cc->L); memset(&cc->J, 0, sizeof cc->J);
    clh::CcLaunch& L = cc->L;
    L.max_chains = max_chains; L.slots = max_chains > 1 ? max_chains - 1 : 1; L.k = x->k; L.n_contigs = (int32_t)x->c_off.size(); L.max_span = cc->jo->max_span;
    L.min_path_score = cc->min_path_score;
    cc->slots_max = (size_t)reads_max * (size_t)L.slots;
    cc->site.assign(clh::kJxSites, 0);
    sp_table(cc->sp, cc->site.data());
    L.read_off = B.put(cc->h_roff);
    L.genome = (const uint8_t*)x->genome->d_codes; L.ctg_off = x->d_coff; L.ctg_len = x->d_clen;
    L.sel = B.get<int64_t>((size_t)clh::kCcSel * (size_t)reads_max);
    L.task = B.get<int64_t>((size_t)clh::kJxTask * cc->slots_max);
    L.cls = B.get<int32_t>(cc->slots_max);
    L.count = B.get<unsigned long long>(2 * clh::kJxClasses);
    L.order = B.get<int64_t>(cc->slots_max);
    cc->d_jout = B.get<int64_t>((size_t)clh::kJxRow * cc->slots_max);
    L.junction = cc->d_jout;
    L.circle = B.get<int64_t>((size_t)clh::kCcRow * (size_t)n);
    const int32_t* d_site = B.put(cc->site);
    if (!L.read_off || !L.sel || !L.task || !L.cls || !L.count || !L.order || !cc->d_jout || !L.circle || !d_site) return sd_refused(me, B);
    HIPCHK(hipMemsetAsync(L.circle, 0x80, sizeof(int64_t) * clh::kCcRow * (size_t)n, st));
    clh::JxLaunch& J = cc->J;
    J.genome = L.genome; J.ctg_off = L.ctg_off; J.ctg_len = L.ctg_len;
    J.reads = (const int8_t*)d_reads; J.read_off = L.read_off; J.task = L.task; J.order = L.order; J.site = d_site; J.out = cc->d_jout;
    const clh_junction_opts* o = cc->jo;
    J.match = o->match; J.mismatch = o->mismatch; J.go = o->gap_open; J.ge = o->gap_extend; J.io = cc->sp->intron_open; J.slack = o->slack; J.max_span = o->max_span;
    return 0;
}

// reads [a, b) of the batch, whose chain and link rows the two kernels in front have just left on the device: the best path and its tasks,
// the class routing, K7j on them, the circle rows.  One copy of kJxClasses counters comes back in between: the junction launches are sized by them.
static int cc_share(const std::string& me, clh_seed_index* x, SdCircle* cc, const clh::ChParams& C, const clh::LkLaunch& K, int32_t a, int32_t b)
{
    hipStream_t st = x->ctx->stream;
    clh::CcLaunch& L = cc->L;
    L.seg = C.seg; L.rows = C.rows; L.lseg = K.lseg; L.lrows = K.lrows; L.nreads = b - a; L.read0 = a;
    const size_t slots = (size_t)L.nreads * (size_t)L.slots;
    HIPCHK(hipMemsetAsync(L.count, 0, sizeof(unsigned long long) * 2 * clh::kJxClasses, st));
    HIPCHK(hipMemsetAsync(L.sel, 0x80, sizeof(int64_t) * clh::kCcSel * (size_t)L.nreads, st));
    HIPCHK(hipMemsetAsync(cc->d_jout, 0x80, sizeof(int64_t) * clh::kJxRow * slots, st));
    HIPCHK(hipEventRecord(x->cev[0], st));
    HIPCHK(clh::launch_seed_circle_select(L, st));
    HIPCHK(clh::launch_seed_circle_route(L, st));
    HIPCHK(hipEventRecord(x->cev[1], st));
    HIPCHK(hipMemcpyAsync(cc->h_count, L.count, sizeof(unsigned long long) * clh::kJxClasses, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    clh::JxLaunch& J = cc->J;
    J.first[0] = 0;
    for (int c = 0; c < clh::kJxClasses; ++c) J.first[c + 1] = J.first[c] + (int64_t)cc->h_count[c];
    if (J.first[clh::kJxClasses] < 0 || (size_t)J.first[clh::kJxClasses] > slots)
        return fail(CLH_E_HIP, me + "the select kernel counted " + std::to_string(J.first[clh::kJxClasses]) + " tasks in " + std::to_string(slots) + " slots");
    cc->h_total += J.first[clh::kJxClasses];
    HIPCHK(hipEventRecord(x->cev[2], st));
    HIPCHK(clh::launch_seed_junction(J, st));
    HIPCHK(hipEventRecord(x->cev[3], st));
    HIPCHK(clh::launch_seed_circle_finalise(L, st));
    HIPCHK(hipEventRecord(x->cev[4], st));
    return 0;
}

// after the last share: the table of the whole batch's rows, and everything that goes back to the host
static int cc_table(const std::string& me, clh_seed_index* x, SdBlocks& B, int32_t n, SdCircle* cc)
{
    hipStream_t st = x->ctx->stream;
    *cc->n_circles = 0;
    x->h_table.clear();
    if (n <= 0) return 0;
    const size_t N = (size_t)n;
    const int64_t* d_circle = cc->L.circle;
    uint64_t* d_w[5];                                   // key_lo, key_hi, reads; two more for the sorts' outputs
    for (auto& p : d_w) p = B.get<uint64_t>(N);
    uint64_t* d_perm = B.get<uint64_t>(N);
    int32_t* d_head = B.get<int32_t>(N + 1);
    int64_t* d_first = B.get<int64_t>(N + 1);
    int64_t* d_table = B.get<int64_t>((size_t)clh::kCcTable * N);
    int64_t* d_cor = B.get<int64_t>(N);
    const size_t sb = clh::seed_sort_temp_bytes(n), tb = clh::seed_scan_temp_bytes(n + 1);
    void* d_sort = B.get<uint8_t>(sb);
    void* d_scan = B.get<uint8_t>(tb);
    if (!d_w[0] || !d_w[1] || !d_w[2] || !d_w[3] || !d_w[4] || !d_perm || !d_head || !d_first || !d_table || !d_cor || !d_sort || !d_scan) return sd_refused(me, B);
    HIPCHK(hipMemsetAsync(d_cor, 0x80, sizeof(int64_t) * N, st));
    HIPCHK(hipEventRecord(x->cev[5], st));
    HIPCHK(clh::launch_seed_circle_keys(d_circle, n, d_w[0], d_w[1], d_w[2], st));
    // least significant first: (end, strand), then (contig, start) with the rows of another status last; both sorts stable
    HIPCHK(clh::seed_sort_pairs(d_sort, sb, d_w[0], d_w[3], d_w[2], d_w[4], n, 42, st));
    HIPCHK(clh::launch_seed_circle_gather(d_w[1], d_w[4], n, d_w[0], st));
    HIPCHK(clh::seed_sort_pairs(d_sort, sb, d_w[0], d_w[3], d_w[4], d_perm, n, 64, st));
    HIPCHK(clh::launch_seed_circle_heads(d_circle, d_perm, n, d_head, st));
    HIPCHK(clh::seed_scan_counts(d_scan, tb, d_head, d_first, (int64_t)n + 1, st));
    HIPCHK(clh::launch_seed_circle_table(d_circle, d_perm, d_head, d_first, n, d_table, d_cor, st));
    HIPCHK(hipEventRecord(x->cev[6], st));
    int64_t groups = 0;
    HIPCHK(hipMemcpyAsync(&groups, d_first + n, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(cc->circle_out, d_circle, sizeof(int64_t) * clh::kCcRow * N, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(cc->cor_out, d_cor, sizeof(int64_t) * N, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    float t = 0;
    HIPCHK(hipEventElapsedTime(&t, x->cev[5], x->cev[6]));
    cc->ms[2] += t;
    if (groups < 0 || groups > n) return fail(CLH_E_HIP, me + "the table step left " + std::to_string(groups) + " circles of " + std::to_string(n) + " reads");
    int64_t found = 0;
    for (int32_t r = 0; r < n; ++r) {
        const int64_t* c = cc->circle_out + (size_t)clh::kCcRow * (size_t)r;
        if (c[0] < clh::kCcFound || c[0] > clh::kCcNoJunction || c[15] != 0)
            return fail(CLH_E_HIP, me + "the circle kernels left read " + std::to_string(r) + (c[0] == clh::kChUnwritten ? " unwritten" : " with status " + std::to_string(c[0])));
        const int64_t g = cc->cor_out[r];
        if (c[0] == clh::kCcFound ? (g < 0 || g >= groups) : g != -1) return fail(CLH_E_HIP, me + "the table step left read " + std::to_string(r) + " in row " + std::to_string(g));
        found += c[0] == clh::kCcFound;
    }
    if ((found > 0) != (groups > 0)) return fail(CLH_E_HIP, me + "the table step left " + std::to_string(groups) + " circles of " + std::to_string(found) + " reads with one");
    x->h_table.assign((size_t)clh::kCcTable * (size_t)groups, 0);
    if (groups > 0) HIPCHK(hipMemcpy(x->h_table.data(), d_table, sizeof(int64_t) * clh::kCcTable * (size_t)groups, hipMemcpyDeviceToHost));
    *cc->n_circles = groups;
    return 0;
}

// seeds, and chains where o is given, and their links where lo is: the anchors and the chain rows of a share stay on the device between the steps
static int sd_seeds(const std::string& me, clh_seed_index* x, int32_t n, const int8_t* reads, const int64_t* read_off, int64_t workspace_bytes, int64_t* anchor_off,
                    int32_t* repetitive, const clh_chain_opts* o, int64_t* seg_out, int64_t* rows_out, const clh_link_opts* lo = nullptr, int64_t* lseg_out = nullptr,
                    int64_t* lrows_out = nullptr, SdCircle* cc = nullptr)
{
    clh_ctx* ctx = x->ctx;
    hipStream_t st = ctx->stream;
    SdReads R;                                          // before B: see SdEntries
    std::vector<int64_t> rm, ra;
    std::vector<int32_t> rrep;
    SdBlocks B(ctx);
    if (int rc = sd_reads(me, x, B, n, reads, read_off, &R)) return rc;
    const int64_t nmin = R.E.n;
    int64_t* d_lo = B.get<int64_t>((size_t)nmin);
    int32_t* d_cnt = B.get<int32_t>((size_t)nmin + 1);
    uint8_t* d_rep = B.get<uint8_t>((size_t)nmin);
    int64_t* d_aoff = B.get<int64_t>((size_t)nmin + 1);
    int64_t* d_rlen = B.put(R.len);
    int64_t* d_rm = B.get<int64_t>((size_t)n + 1);
    int64_t* d_ra = B.get<int64_t>((size_t)n + 1);
    int32_t* d_rrep = B.get<int32_t>((size_t)n);
    const size_t tb = clh::seed_scan_temp_bytes(nmin + 1);
    void* d_temp = B.get<uint8_t>(tb);
    if (!d_lo || !d_cnt || !d_rep || !d_aoff || !d_rlen || !d_rm || !d_ra || !d_rrep || !d_temp) return sd_refused(me, B);
    HIPCHK(hipMemsetAsync(d_cnt, 0, sizeof(int32_t) * ((size_t)nmin + 1), st));
    HIPCHK(clh::launch_seed_lookup(x->d_keys, x->n, x->max_occ, R.E.keys, nmin, d_lo, d_cnt, d_rep, st));
    HIPCHK(clh::seed_scan_counts(d_temp, tb, d_cnt, d_aoff, nmin + 1, st));
    HIPCHK(clh::launch_seed_per_read(R.E.d_seq_item0, R.E.d_item_off, d_aoff, d_rep, n, d_rm, d_ra, d_rrep, st));
    HIPCHK(hipEventRecord(x->ev[1], st));
    rm.resize((size_t)n + 1); ra.resize((size_t)n + 1); rrep.resize((size_t)n);
    HIPCHK(hipMemcpyAsync(rm.data(), d_rm, sizeof(int64_t) * ((size_t)n + 1), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(ra.data(), d_ra, sizeof(int64_t) * ((size_t)n + 1), hipMemcpyDeviceToHost, st));
    if (n > 0) HIPCHK(hipMemcpyAsync(rrep.data(), d_rrep, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    float t = 0;
    HIPCHK(hipEventElapsedTime(&t, x->ev[0], x->ev[1]));
    x->ms[2] = t;
    if (o) x->ms[3] = 0;
    if (lo) x->ms[4] = 0;
    // shares of whole reads, 64 bytes an anchor: four sort words, the sort's own space, f, p and the used mark
    const int64_t ws = workspace_bytes > 0 ? workspace_bytes : (int64_t)1 << 30, cap = ws / 64;
    std::vector<int32_t> cut(1, 0);
    int64_t share_max = 0;
    int32_t reads_max = 0;
    for (int32_t a = 0; a < n;) {
        int32_t b = a;
        while (b < n && ra[b + 1] - ra[a] <= cap) ++b;
        if (b == a)
            return fail(CLH_E_CAPACITY, me + "read " + std::to_string(a) + " alone has " + std::to_string(ra[a + 1] - ra[a]) + " anchors, workspace_bytes holds " +
                                            std::to_string(cap));
        share_max = std::max(share_max, ra[b] - ra[a]); reads_max = std::max(reads_max, b - a);
        cut.push_back(b); a = b;
    }
    x->last_shares = (int)cut.size() - 1;
    const int64_t total = ra[n];
    if (!o) {
        x->h_k1.assign((size_t)total, 0); x->h_k2.assign((size_t)total, 0);
        for (int32_t r = 0; r <= n; ++r) anchor_off[r] = ra[r];
        for (int32_t r = 0; r < n; ++r) repetitive[r] = rrep[r];
    }
    uint64_t* d_k[4];
    for (auto& p : d_k) p = B.get<uint64_t>((size_t)share_max);
    const size_t sb = clh::seed_sort_temp_bytes(share_max);
    void* d_sort = B.get<uint8_t>(sb);
    if (!d_k[0] || !d_k[1] || !d_k[2] || !d_k[3] || !d_sort) return sd_refused(me, B);
    clh::ChParams C;
    memset(&C, 0, sizeof C);
    size_t seg_bytes = 0, row_bytes = 0;
    if (o) {
        C.ctg_off = x->d_coff; C.ctg_len = x->d_clen; C.n_contigs = (int32_t)x->c_off.size();
        C.k = x->k; C.lookback = o->lookback; C.max_chains = o->max_chains; C.max_attempts = o->max_attempts; C.min_score = o->min_score; C.min_anchors = o->min_anchors;
        C.max_gap = o->max_gap; C.max_skew = o->max_skew;
        seg_bytes = sizeof(int64_t) * clh::kChSeg * 2 * (size_t)reads_max; row_bytes = sizeof(int64_t) * clh::kChRow * (size_t)o->max_chains * 2 * (size_t)reads_max;
        C.seg_bounds = B.get<int64_t>(2 * (size_t)reads_max + 1);
        C.f = B.get<int32_t>((size_t)share_max); C.p = B.get<int32_t>((size_t)share_max); C.used = B.get<uint8_t>((size_t)share_max);
        C.seg = (int64_t*)B.get<uint8_t>(seg_bytes); C.rows = (int64_t*)B.get<uint8_t>(row_bytes);
        if (!C.seg_bounds || !C.f || !C.p || !C.used || !C.seg || !C.rows) return sd_refused(me, B);
    }
    clh::LkLaunch K;
    memset(&K, 0, sizeof K);
    if (lo) {
        K.seg = C.seg; K.rows = C.rows; K.max_chains = o->max_chains; K.k = x->k; K.p = lk_params(lo);
        K.lseg = B.get<int64_t>((size_t)clh::kLkSeg * 2 * (size_t)reads_max); K.lrows = B.get<int64_t>((size_t)clh::kLkRow * (size_t)o->max_chains * 2 * (size_t)reads_max);
        if (!K.lseg || !K.lrows) return sd_refused(me, B);
    }
    if (cc)
        if (int rc = cc_prepare(me, x, B, R.d_codes, n, reads_max, o->max_chains, cc)) return rc;
    const int bits_x = sd_bits((uint64_t)(x->genome->len > 0 ? x->genome->len : 1)) + clh::kSdYBits, bits_r = sd_bits(2 * (uint64_t)(n > 0 ? n : 1));
    for (size_t s = 0; s + 1 < cut.size(); ++s) {
        const int32_t a = cut[s], b = cut[s + 1];
        const int64_t A = ra[b] - ra[a];
        HIPCHK(hipEventRecord(x->ev[0], st));
        HIPCHK(clh::launch_seed_anchor_fill(x->d_vals, x->n, R.E.vals, R.E.seq_of, d_rlen, d_lo, d_cnt, d_aoff, rm[a], rm[b], ra[a], x->k, d_k[0], d_k[1], A, st));
        // least significant first: (x, y), then (read, minus); both sorts stable
        HIPCHK(clh::seed_sort_pairs(d_sort, sb, d_k[1], d_k[3], d_k[0], d_k[2], A, bits_x, st));
        HIPCHK(clh::seed_sort_pairs(d_sort, sb, d_k[2], d_k[0], d_k[3], d_k[1], A, bits_r, st));
        HIPCHK(hipEventRecord(x->ev[1], st));
        if (!o) {
            if (A > 0) {
                HIPCHK(hipMemcpyAsync(x->h_k1.data() + ra[a], d_k[0], sizeof(uint64_t) * (size_t)A, hipMemcpyDeviceToHost, st));
                HIPCHK(hipMemcpyAsync(x->h_k2.data() + ra[a], d_k[1], sizeof(uint64_t) * (size_t)A, hipMemcpyDeviceToHost, st));
            }
        } else {
            C.k1 = d_k[0]; C.k2 = d_k[1]; C.n_anchors = A; C.read0 = a; C.nseg = 2 * (b - a);
            const size_t sg = sizeof(int64_t) * clh::kChSeg * (size_t)C.nseg, rw = sizeof(int64_t) * clh::kChRow * (size_t)o->max_chains * (size_t)C.nseg;
            HIPCHK(hipMemsetAsync(C.seg, 0x80, sg, st));
            HIPCHK(hipMemsetAsync(C.rows, 0x80, rw, st));
            HIPCHK(clh::launch_seed_segments(C, st));
            HIPCHK(clh::launch_seed_chain(C, st));
            HIPCHK(hipEventRecord(x->ev[2], st));
            if (lo) {                                   // on the device rows, directly behind the chain kernel
                const size_t lsg = sizeof(int64_t) * clh::kLkSeg * (size_t)C.nseg, lrw = sizeof(int64_t) * clh::kLkRow * (size_t)o->max_chains * (size_t)C.nseg;
                K.nseg = C.nseg;
                HIPCHK(hipMemsetAsync(K.lseg, 0x80, lsg, st));
                HIPCHK(hipMemsetAsync(K.lrows, 0x80, lrw, st));
                HIPCHK(hipEventRecord(x->ev[4], st));     // the link slot times the kernel alone, not the marker fill
                HIPCHK(clh::launch_seed_link(K, st));
                HIPCHK(hipEventRecord(x->ev[3], st));
                if (cc) {                               // the rows stay where they are: select, tasks, K7j and the circle rows behind the link kernel
                    if (int rc = cc_share(me, x, cc, C, K, a, b)) return rc;
                } else {
                    HIPCHK(hipMemcpyAsync(lseg_out + (size_t)clh::kLkSeg * 2 * (size_t)a, K.lseg, lsg, hipMemcpyDeviceToHost, st));
                    HIPCHK(hipMemcpyAsync(lrows_out + (size_t)clh::kLkRow * (size_t)o->max_chains * 2 * (size_t)a, K.lrows, lrw, hipMemcpyDeviceToHost, st));
                }
            }
            if (!cc) {
                HIPCHK(hipMemcpyAsync(seg_out + (size_t)clh::kChSeg * 2 * (size_t)a, C.seg, sg, hipMemcpyDeviceToHost, st));
                HIPCHK(hipMemcpyAsync(rows_out + (size_t)clh::kChRow * (size_t)o->max_chains * 2 * (size_t)a, C.rows, rw, hipMemcpyDeviceToHost, st));
            }
        }
        HIPCHK(hipStreamSynchronize(st));
        if (cc) {
            HIPCHK(hipEventElapsedTime(&t, x->cev[0], x->cev[1])); cc->ms[0] += t;
            HIPCHK(hipEventElapsedTime(&t, x->cev[2], x->cev[3])); cc->ms[1] += t;
            HIPCHK(hipEventElapsedTime(&t, x->cev[3], x->cev[4])); cc->ms[2] += t;
        }
        HIPCHK(hipEventElapsedTime(&t, x->ev[0], x->ev[1]));
        x->ms[2] += t;
        if (o) { HIPCHK(hipEventElapsedTime(&t, x->ev[1], x->ev[2])); x->ms[3] += t; }
        if (lo) { HIPCHK(hipEventElapsedTime(&t, x->ev[4], x->ev[3])); x->ms[4] += t; }
    }
    if (cc) return cc_table(me, x, B, n, cc);          // the select kernel checked the headers and rows where they lay
    if (o)
        for (int64_t s = 0; s < 2 * (int64_t)n; ++s) {
            const int64_t* h = seg_out + clh::kChSeg * s;
            if (h[0] == clh::kChUnwritten || h[0] < 0 || h[0] > o->max_chains || h[3] != 0)
                return fail(CLH_E_HIP, me + "the chain kernel left segment " + std::to_string(s) + (h[0] == clh::kChUnwritten ? " unwritten" : " with status " + std::to_string(h[3])));
            for (int64_t c = 0; c < h[0]; ++c)
                if (rows_out[((s * o->max_chains) + c) * clh::kChRow + 9] != 0) return fail(CLH_E_HIP, me + "the chain kernel left a row of segment " + std::to_string(s) + " unwritten");
        }
    if (lo) return lk_validate(me, 0, 2 * (int64_t)n, o->max_chains, seg_out, lseg_out, lrows_out);
    return 0;
}

extern "C" int clh_seed_batch(clh_seed_index* x, int32_t n, const int8_t* reads, const int64_t* read_off, int64_t workspace_bytes, int64_t* anchor_off,
                              int32_t* repetitive)
{
    const std::string me = "clh_seed_batch: ";
    if (!x || !anchor_off || (n > 0 && !repetitive)) return fail(CLH_E_ARG, me + "null argument");
    x->h_k1.clear(); x->h_k2.clear();
    const int rc = sd_seeds(me, x, n, reads, read_off, workspace_bytes, anchor_off, repetitive, nullptr, nullptr, nullptr);
    if (rc) { x->h_k1.clear(); x->h_k2.clear(); }
    return rc;
}

extern "C" int clh_seed_batch_fetch(clh_seed_index* x, int64_t cap, int32_t* read, uint8_t* minus, int64_t* xs, int32_t* ys)
{
    if (!x) return fail(CLH_E_ARG, "clh_seed_batch_fetch: null argument");
    const int64_t m = (int64_t)x->h_k1.size();
    if (cap < m) return fail(CLH_E_CAPACITY, "clh_seed_batch_fetch: cap too small");
    if (m > 0 && (!read || !minus || !xs || !ys)) return fail(CLH_E_ARG, "clh_seed_batch_fetch: null argument");
    for (int64_t i = 0; i < m; ++i) {
        read[i] = (int32_t)(x->h_k1[i] >> 1); minus[i] = (uint8_t)(x->h_k1[i] & 1);
        xs[i] = (int64_t)(x->h_k2[i] >> clh::kSdYBits); ys[i] = (int32_t)(x->h_k2[i] & (((uint64_t)1 << clh::kSdYBits) - 1));
    }
    return 0;
}

extern "C" int clh_seed_chain_batch(clh_seed_index* x, int32_t n, const int8_t* reads, const int64_t* read_off, const clh_chain_opts* o, int64_t* seg, int64_t* rows)
{
    const std::string me = "clh_seed_chain_batch: ";
    if (!x || !o || (n > 0 && (!seg || !rows))) return fail(CLH_E_ARG, me + "null argument");
    if (o->lookback < 1 || o->lookback > clh::kChLookbackMax) return fail(CLH_E_ARG, me + "lookback must be 1..64");
    if (o->max_chains < 1 || o->max_chains > clh::kChMaxChains) return fail(CLH_E_ARG, me + "max_chains must be 1..64");
    if (o->max_attempts < 1 || o->max_gap < 0 || o->max_skew < 0) return fail(CLH_E_ARG, me + "max_attempts must be at least 1, max_gap and max_skew not negative");
    return sd_seeds(me, x, n, reads, read_off, o->workspace_bytes, nullptr, nullptr, o, seg, rows);
}

extern "C" int clh_seed_link_batch(clh_seed_index* x, int32_t n, const int8_t* reads, const int64_t* read_off, const clh_chain_opts* o, const clh_link_opts* lo,
                                   int64_t* seg, int64_t* rows, int64_t* link_seg, int64_t* link_rows)
{
    const std::string me = "clh_seed_link_batch: ";
    if (!x || !o || !lo || (n > 0 && (!seg || !rows || !link_seg || !link_rows))) return fail(CLH_E_ARG, me + "null argument");
    if (o->lookback < 1 || o->lookback > clh::kChLookbackMax) return fail(CLH_E_ARG, me + "lookback must be 1..64");
    if (o->max_chains < 1 || o->max_chains > clh::kChMaxChains) return fail(CLH_E_ARG, me + "max_chains must be 1..64");
    if (o->max_attempts < 1 || o->max_gap < 0 || o->max_skew < 0) return fail(CLH_E_ARG, me + "max_attempts must be at least 1, max_gap and max_skew not negative");
    if (int rc = lk_opts_check(me, lo)) return rc;
    return sd_seeds(me, x, n, reads, read_off, o->workspace_bytes, nullptr, nullptr, o, seg, rows, lo, link_seg, link_rows);
}

extern "C" int clh_seed_link_rows(clh_seed_index* x, int32_t nseg, int32_t max_chains, const int64_t* seg, const int64_t* rows, const clh_link_opts* lo,
                                  int64_t* link_seg, int64_t* link_rows)
{
    const std::string me = "clh_seed_link_rows: ";
    if (!x || !lo || nseg < 0 || (nseg > 0 && (!seg || !rows || !link_seg || !link_rows))) return fail(CLH_E_ARG, me + "null argument");
    if (max_chains < 1 || max_chains > clh::kChMaxChains) return fail(CLH_E_ARG, me + "max_chains must be 1..64");
    if (int rc = lk_opts_check(me, lo)) return rc;
    for (int64_t s = 0; s < nseg; ++s) {
        const int64_t nc = seg[clh::kChSeg * s];
        if (nc < 0 || nc > max_chains) return fail(CLH_E_ARG, me + "segment " + std::to_string(s) + " has " + std::to_string(nc) + " chains, outside 0.." + std::to_string(max_chains));
        for (int64_t c = 0; c < nc; ++c) {
            const int64_t* r = rows + (s * max_chains + c) * clh::kChRow;
            for (int f = 5; f <= 8; ++f)
                if (r[f] < 0 || r[f] >= clh::kLkLimit) return fail(CLH_E_ARG, me + "segment " + std::to_string(s) + ", chain " + std::to_string(c) + ": a coordinate outside [0, 2^40)");
            if (r[3] <= -clh::kLkLimit || r[3] >= clh::kLkLimit) return fail(CLH_E_ARG, me + "segment " + std::to_string(s) + ", chain " + std::to_string(c) + ": a score outside (-2^40, 2^40)");
        }
    }
    x->ms[4] = 0;
    if (nseg == 0) return 0;
    HIPCHK(hipSetDevice(x->ctx->device));
    hipStream_t st = x->ctx->stream;
    SdBlocks B(x->ctx);                                 // seg and rows are the caller's and outlive the call; the copies are drained by B
    const size_t sg = (size_t)clh::kChSeg * (size_t)nseg, rw = (size_t)clh::kChRow * (size_t)max_chains * (size_t)nseg;
    const size_t lsg = (size_t)clh::kLkSeg * (size_t)nseg, lrw = (size_t)clh::kLkRow * (size_t)max_chains * (size_t)nseg;
    int64_t* d_seg = B.get<int64_t>(sg); int64_t* d_rows = B.get<int64_t>(rw);
    clh::LkLaunch K;
    memset(&K, 0, sizeof K);
    K.lseg = B.get<int64_t>(lsg); K.lrows = B.get<int64_t>(lrw);
    if (!d_seg || !d_rows || !K.lseg || !K.lrows) return sd_refused(me, B);
    K.seg = d_seg; K.rows = d_rows; K.nseg = nseg; K.max_chains = max_chains; K.k = x->k; K.p = lk_params(lo);
    HIPCHK(hipMemcpyAsync(d_seg, seg, sizeof(int64_t) * sg, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_rows, rows, sizeof(int64_t) * rw, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(K.lseg, 0x80, sizeof(int64_t) * lsg, st));
    HIPCHK(hipMemsetAsync(K.lrows, 0x80, sizeof(int64_t) * lrw, st));
    HIPCHK(hipEventRecord(x->ev[2], st));
    HIPCHK(clh::launch_seed_link(K, st));
    HIPCHK(hipEventRecord(x->ev[3], st));
    HIPCHK(hipMemcpyAsync(link_seg, K.lseg, sizeof(int64_t) * lsg, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(link_rows, K.lrows, sizeof(int64_t) * lrw, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipEventElapsedTime(&x->ms[4], x->ev[2], x->ev[3]));
    return lk_validate(me, 0, nseg, max_chains, seg, link_seg, link_rows);
}

// ---- K7j: back-splice junctions refined to the base (seed_junction.hip; the definitions in seed_device.h and the header) ----------
static_assert(clh::kJxSiteOther == clh::kSpOther && clh::kJxSites == clh::kSpSites, "K7j reads the spliced kernels' site table");

extern "C" int clh_seed_junction_info(int64_t* out)
{
    if (!out) return fail(CLH_E_ARG, "clh_seed_junction_info: null argument");
    static_assert(clh::kJxClasses == 4, "out[0..3] are the class bounds");
    const int64_t v[8] = {clh::jx_class_bound(0), clh::jx_class_bound(1), clh::jx_class_bound(2), clh::jx_class_bound(3), clh::kJxMaxSpan, clh::kJxMaxSlack,
                          clh::kJxWaves, clh::kJxClasses};
    for (int i = 0; i < 8; ++i) out[i] = v[i];
    return 0;
}

extern "C" int clh_seed_junction_batch(clh_seed_index* x, int32_t n_reads, const int8_t* reads, const int64_t* read_off, int64_t n_tasks, const int64_t* task,
                                       const clh_junction_opts* o, const clh_splice* sp, int64_t* out, float* kernel_ms)
{
    const std::string me = "clh_seed_junction_batch: ";
    if (kernel_ms) *kernel_ms = 0;
    if (!x || !o || !sp || n_reads < 0 || n_tasks < 0 || !read_off || (n_tasks > 0 && (!task || !out))) return fail(CLH_E_ARG, me + "null argument");
    if (int rc = jx_opts_check(me, o, sp)) return rc;
    if (read_off[0] < 0) return fail(CLH_E_ARG, me + "offsets must ascend from 0 or above");
    for (int32_t r = 0; r < n_reads; ++r)
        if (read_off[r + 1] < read_off[r]) return fail(CLH_E_ARG, me + "offsets must ascend");
    if (read_off[n_reads] > 0 && !reads) return fail(CLH_E_ARG, me + "null argument");
    for (int32_t r = 0; r < n_reads; ++r)
        for (int64_t i = read_off[r]; i < read_off[r + 1]; ++i)
            if (reads[i] < 0 || reads[i] > 4) return fail(CLH_E_ARG, me + "read " + std::to_string(r) + " holds a code outside 0..4");
    const int64_t n_ctg = (int64_t)x->c_off.size();
    std::vector<int64_t> order((size_t)n_tasks);        // before B: see SdEntries
    std::vector<int32_t> site(clh::kJxSites);
    clh::JxLaunch K;
    memset(&K, 0, sizeof K);
    std::vector<int8_t> cls((size_t)n_tasks);
    int64_t count[clh::kJxClasses] = {0, 0, 0, 0};
    for (int64_t t = 0; t < n_tasks; ++t) {
        const int64_t* k = task + clh::kJxTask * t;
        const std::string who = me + "task " + std::to_string(t) + ": ";
        if (k[0] < 0 || k[0] >= n_reads) return fail(CLH_E_ARG, who + "read " + std::to_string(k[0]) + " outside the " + std::to_string(n_reads) + " reads");
        if (k[2] < 0 || k[2] >= n_ctg) return fail(CLH_E_ARG, who + "contig " + std::to_string(k[2]) + " outside the " + std::to_string(n_ctg) + " contigs");
        const int64_t L = read_off[k[0] + 1] - read_off[k[0]], len = x->c_len[(size_t)k[2]];
        if (k[4] < 0 || k[4] > L || k[6] < 0 || k[6] > L) return fail(CLH_E_ARG, who + "yd or ya outside [0, " + std::to_string(L) + "]");
        if (k[3] < 0 || k[3] > len || k[5] < 0 || k[5] > len) return fail(CLH_E_ARG, who + "xd or xa outside [0, " + std::to_string(len) + "]");
        if (k[7] < -1 || k[7] > 1) return fail(CLH_E_ARG, who + "strand must be -1, 0 or +1, got " + std::to_string(k[7]));
        cls[(size_t)t] = (int8_t)(clh::jx_status(k[3], k[4], k[5], k[6], o->max_span) ? 0 : clh::jx_class(k[6] - k[4]));
        ++count[cls[(size_t)t]];
    }
    if (n_tasks == 0) return 0;
    int64_t next[clh::kJxClasses];
    for (int c = 0; c < clh::kJxClasses; ++c) { K.first[c + 1] = K.first[c] + count[c]; next[c] = K.first[c]; }
    for (int64_t t = 0; t < n_tasks; ++t) order[(size_t)next[cls[(size_t)t]]++] = t;
    sp_table(sp, site.data());
    HIPCHK(hipSetDevice(x->ctx->device));
    hipStream_t st = x->ctx->stream;
    SdBlocks B(x->ctx);
    const size_t total = (size_t)read_off[n_reads], nt = (size_t)n_tasks;
    int8_t* d_reads = B.get<int8_t>(total);
    int64_t* d_roff = B.get<int64_t>((size_t)n_reads + 1);
    int64_t* d_task = B.get<int64_t>(nt * clh::kJxTask);
    K.order = B.put(order); K.site = B.put(site);
    K.out = B.get<int64_t>(nt * clh::kJxRow);
    if (!d_reads || !d_roff || !d_task || !K.order || !K.site || !K.out) return sd_refused(me, B);
    if (total) HIPCHK(hipMemcpyAsync(d_reads, reads, total, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_roff, read_off, sizeof(int64_t) * ((size_t)n_reads + 1), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_task, task, sizeof(int64_t) * nt * clh::kJxTask, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(K.out, 0x80, sizeof(int64_t) * nt * clh::kJxRow, st));
    K.genome = (const uint8_t*)x->genome->d_codes; K.ctg_off = x->d_coff; K.ctg_len = x->d_clen;
    K.reads = d_reads; K.read_off = d_roff; K.task = d_task;
    K.match = o->match; K.mismatch = o->mismatch; K.go = o->gap_open; K.ge = o->gap_extend; K.io = sp->intron_open; K.slack = o->slack; K.max_span = o->max_span;
    HIPCHK(hipEventRecord(x->ev[2], st));
    HIPCHK(clh::launch_seed_junction(K, st));
    HIPCHK(hipEventRecord(x->ev[3], st));
    HIPCHK(hipMemcpyAsync(out, K.out, sizeof(int64_t) * nt * clh::kJxRow, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, x->ev[2], x->ev[3]));
    if (kernel_ms) *kernel_ms = ms;
    for (int64_t t = 0; t < n_tasks; ++t) {
        const int64_t* r = out + clh::kJxRow * t;
        const int64_t* k = task + clh::kJxTask * t;
        if (r[0] == clh::kChUnwritten || r[0] != clh::jx_status(k[3], k[4], k[5], k[6], o->max_span))
            return fail(CLH_E_HIP, me + "the junction kernel left task " + std::to_string(t) + (r[0] == clh::kChUnwritten ? " unwritten" : " with status " + std::to_string(r[0])));
        if (r[0] == 0 && (r[3] < 0 || r[3] > k[6] - k[4] || r[4] < 0 || r[5] < 0 || r[6] > x->c_len[(size_t)k[2]] || r[7] < 0 || r[7] >= r[6]))
            return fail(CLH_E_HIP, me + "the junction kernel left the row of task " + std::to_string(t) + " out of range");
    }
    return 0;
}

// ---- K7c: the circles of a read batch in one device pass (seed_circle.hip; the definitions in seed_device.h and the header) --------
extern "C" int clh_seed_circle_batch(clh_seed_index* x, int32_t n, const int8_t* reads, const int64_t* read_off, const clh_chain_opts* o, const clh_link_opts* lo,
                                     const clh_junction_opts* jo, const clh_splice* sp, int64_t min_path_score, int64_t* circle, int64_t* circle_of_read,
                                     int64_t* n_circles, float* kernel_ms)
{
    const std::string me = "clh_seed_circle_batch: ";
    if (kernel_ms) kernel_ms[0] = kernel_ms[1] = kernel_ms[2] = 0;
    if (!x || !o || !lo || !jo || !sp || !n_circles || !read_off || n < 0 || (n > 0 && (!circle || !circle_of_read))) return fail(CLH_E_ARG, me + "null argument");
    *n_circles = 0;
    x->h_table.clear();
    if (o->lookback < 1 || o->lookback > clh::kChLookbackMax) return fail(CLH_E_ARG, me + "lookback must be 1..64");
    if (o->max_chains < 1 || o->max_chains > clh::kChMaxChains) return fail(CLH_E_ARG, me + "max_chains must be 1..64");
    if (o->max_attempts < 1 || o->max_gap < 0 || o->max_skew < 0) return fail(CLH_E_ARG, me + "max_attempts must be at least 1, max_gap and max_skew not negative");
    if (int rc = lk_opts_check(me, lo)) return rc;
    if (int rc = jx_opts_check(me, jo, sp)) return rc;
    if (x->c_off.size() >= ((size_t)1 << clh::kCcContigBits)) return fail(CLH_E_CAPACITY, me + "an index of 2^23 contigs or more: the table's sort word holds 23 bits of them");
    if (n == 0) return read_off[0] < 0 ? fail(CLH_E_ARG, me + "offsets must ascend from 0 or above") : 0;
    SdCircle cc;                                        // before sd_seeds' SdBlocks: see SdEntries
    cc.jo = jo; cc.sp = sp; cc.min_path_score = min_path_score; cc.circle_out = circle; cc.cor_out = circle_of_read; cc.n_circles = n_circles;
    cc.h_roff.assign(read_off, read_off + (size_t)n + 1);
    const int rc = sd_seeds(me, x, n, reads, read_off, o->workspace_bytes, nullptr, nullptr, o, nullptr, nullptr, lo, nullptr, nullptr, &cc);
    if (rc) { x->h_table.clear(); *n_circles = 0; return rc; }
    if (kernel_ms) for (int i = 0; i < 3; ++i) kernel_ms[i] = cc.ms[i];
    return 0;
}

extern "C" int clh_seed_circle_table_fetch(clh_seed_index* x, int64_t cap, int64_t* table)
{
    if (!x) return fail(CLH_E_ARG, "clh_seed_circle_table_fetch: null argument");
    const int64_t m = (int64_t)(x->h_table.size() / clh::kCcTable);
    if (cap < m) return fail(CLH_E_CAPACITY, "clh_seed_circle_table_fetch: cap too small");
    if (m > 0 && !table) return fail(CLH_E_ARG, "clh_seed_circle_table_fetch: null argument");
    for (size_t i = 0; i < x->h_table.size(); ++i) table[i] = x->h_table[i];
    return 0;
}

// the letters of n spans of the resident genome as codes 0..4 (bits 0-2 of the byte, clamped to 4): one small gather on the device, one
// lane a span, and one copy back -- for the dinucleotides beside many refined junctions, not for windows
extern "C" int clh_genome_letters(clh_genome* g, int32_t n, const int64_t* off, const int64_t* len, int8_t* out)
{
    const std::string me = "clh_genome_letters: ";
    if (!g || n < 0 || (n > 0 && (!off || !len || !out))) return fail(CLH_E_ARG, me + "null argument");
    std::vector<int64_t> at((size_t)n + 1, 0);          // before B: see SdEntries
    for (int i = 0; i < n; ++i) {
        if (off[i] < 0 || len[i] < 0 || off[i] + len[i] > g->len) return fail(CLH_E_ARG, me + "span outside the genome");
        at[(size_t)i + 1] = at[(size_t)i] + len[i];
    }
    const int64_t total = at[(size_t)n];
    if (total == 0) return 0;
    HIPCHK(hipSetDevice(g->ctx->device));
    hipStream_t st = g->ctx->stream;
    SdBlocks B(g->ctx);
    int64_t* d_off = B.get<int64_t>((size_t)n); int64_t* d_len = B.get<int64_t>((size_t)n); int64_t* d_at = B.put(at);
    int8_t* d_out = B.get<int8_t>((size_t)total);
    if (!d_off || !d_len || !d_at || !d_out) return sd_refused(me, B);
    HIPCHK(hipMemcpyAsync(d_off, off, sizeof(int64_t) * (size_t)n, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_len, len, sizeof(int64_t) * (size_t)n, hipMemcpyHostToDevice, st));
    HIPCHK(clh::launch_genome_letters((const uint8_t*)g->d_codes, g->len, d_off, d_len, d_at, n, d_out, st));
    HIPCHK(hipMemcpyAsync(out, d_out, (size_t)total, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}
