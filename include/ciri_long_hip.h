/*
 * ciri_long_hip.h -- C ABI of libclh.so, the MI355X (gfx950) implementation of CIRI-long's per-read hot path.
 *
 * Plain C: pointers and sizes only.  Two groups of entry points:
 *
 *  (1) The six symbols of the reference's libssw.so, with identical signatures, struct layout, ownership and error
 *      conventions, so that the reference's ctypes wrapper (libs/striped_smith_waterman/ssw_wrap.py:54-72,278-288)
 *      can load this library in place of libssw.so.  Declared in ssw_legacy.h.
 *
 *  (2) Batched entry points (this file).  The reference makes one FFI round trip per alignment
 *      (ssw_wrap.py:187-209 <- CIRI_long/find_bsj.py:203-216, CIRI_long/collapse.py:157-173,251-265); a GPU wants
 *      thousands of alignments per launch.  A batch is a pair of packed int8 code arrays (A=0 C=1 G=2 T=3 N=4, the
 *      encoding of ssw_wrap.py:50,243-250) plus offset tables; alignment a is reads[read_off[a]..read_off[a+1]) against
 *      refs[ref_off[a]..ref_off[a+1]).  Results are what n sequential ssw_init+ssw_align calls would return.
 *
 * All functions return 0 on success and a negative CLH_E_* code on failure; clh_last_error() gives the text.
 * There is no CPU fallback: without a usable HIP device every compute entry point fails.
 */
#ifndef CIRI_LONG_HIP_H
#define CIRI_LONG_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)     /* the library itself is built with -fvisibility=hidden: only the C ABI is exported */

#define CLH_E_HIP        (-1)   /* HIP runtime error (no device, launch failure, out of memory) */
#define CLH_E_ARG        (-2)   /* invalid argument */
#define CLH_E_UNSUPPORTED (-3)  /* valid for the reference but not implemented here (see text) */
#define CLH_E_CAPACITY   (-4)   /* caller's output buffer too small */

/* status bits of clh_align_t.status */
#define CLH_ST_WORD        1    /* 16-bit regime (ssw.c:806-809) */
#define CLH_ST_NULL        2    /* the reference would have returned NULL (ssw.c:810-813: score_size 0 overflow) */
#define CLH_ST_TRACE_ERR   4    /* the reference's "Trace back error" (ssw.c:674-682) */
#define CLH_ST_NO_CIGAR    8    /* CIGAR not produced because of flag/filters (ssw.c:834,850) */
#define CLH_ST_CIGAR_TRUNC 16   /* no CIGAR for a capacity reason, scores and coordinates are valid.  DNA (matrix edge 1..5): the
                                 * traceback workspace ran out (retry with a smaller batch), or the band is wider than 2048 cells on an
                                 * aligned reference of more than 2048 bases AND read + reference of the aligned part exceed 12 kB (or the
                                 * read 4096 rows).  Matrix edge 6..32: the final band is wider than 4093 cells on an aligned read of more
                                 * than 5121 letters, or the alignment alone needs more than the whole, empty workspace -- tracebacks the
                                 * shared workspace could not hold during the run are run again in clh_ssw_fetch (see there) */

/* One result row: the fields of s_align (ssw.h:42-52) with the cigar pointer replaced by a slice of the
 * caller's cigar buffer. */
typedef struct {
    uint16_t score1;
    uint16_t score2;
    int32_t ref_begin1;
    int32_t ref_end1;
    int32_t read_begin1;
    int32_t read_end1;
    int32_t ref_end2;
    int32_t cigar_off;    /* first u32 of this alignment's CIGAR in cigar_buf, -1 if none */
    int32_t cigar_len;
    int32_t status;
} clh_align_t;

typedef struct clh_ctx clh_ctx;     /* one per (process, GPU) */
typedef struct clh_plan clh_plan;   /* a batch shape: offsets, scoring, bucketing, device workspaces */

int clh_device_count(void);
const char* clh_last_error(void);
const char* clh_version(void);

clh_ctx* clh_create(int device);    /* NULL on failure */
void clh_destroy(clh_ctx* ctx);
int clh_device_of(const clh_ctx* ctx);

/* Scoring and reporting options; meaning and defaults follow ssw_init/ssw_align (ssw.h:54-120). */
typedef struct {
    const int8_t* mat;     /* n_mat x n_mat substitution matrix, row = reference code (ssw.c:621) */
    int32_t n_mat;         /* 1..32; 6..32 (protein alphabets): the K1a class, packed references only, codes in [0, n_mat) */
    uint8_t gap_open;      /* absolute values, gap_open >= gap_extend required */
    uint8_t gap_extend;
    uint8_t flag;          /* ssw_align flag; ssw_wrap.py always passes 1 */
    int8_t score_size;     /* ssw_init score_size; ssw_wrap.py always passes 2 */
    uint16_t filters;
    int32_t filterd;
    int32_t want_score2;   /* 0: skip the second-best scan (score2 = 0, ref_end2 = 0); CIRI-long never reads it */
    int32_t want_cigar;    /* 0: skip the traceback even if flag asks for it (find_bsj.py:204,214 never reads it) */
} clh_ssw_opts;

/* mask_len may be NULL: ssw_wrap.py:196-199 rule (len/2 if len > 30 else 15). */
clh_plan* clh_ssw_plan(clh_ctx* ctx, int32_t n, const int64_t* read_off, const int64_t* ref_off,
                       const int32_t* mask_len, const clh_ssw_opts* opts);
void clh_plan_destroy(clh_plan* plan);

/* Diagnostics of the last run's CIGAR step (K1b): counts[0] = alignments the row traceback kernel handed to its wide form
 * (bands of 513..2048 cells), counts[1] = alignments that went on to the anti-diagonal kernel (walks that leave the final band,
 * where banded_sw, ssw.c:636-696, reads direction bytes of earlier band iterations; bands above 2048 cells).  Waits for the run. */
int clh_plan_traceback_counts(clh_plan* pl, int32_t* counts);

/* Diagnostics of the exact column prefilter (csrc/ssw_prefilter.hip) in front of the score pass of short reads on long windows --
 * the shape of find_bsj.py:196-216, a 20..254-base clip against hit +- 200 kb: a bit-vector edit-distance bound finds the blocks
 * of the window that can hold the maximum of sw_sse2_byte (ssw.c:123-345) and only those are computed; results are identical with
 * and without it.  out[0] = alignments of that class in the last run, out[1] = of them with candidate slices instead of the
 * whole window, out[2] = slices run, out[3] = window columns computed, out[4] = window columns of the class, out[5] = alignments whose
 * window went through the second stage as well (the indel-distance bound, for windows the first leaves too much of).  Waits for the run. */
int clh_plan_prefilter_stats(clh_plan* pl, int64_t* out);

/* ssw_prefilter_kernel (the first stage) alone, after a run with profiling on: ms[0] / ms[1] = its duration for the class of reads up to
 * 254 bases and for the class of longer reads (0 when it did not run); work[2 c] = window columns x W 32-row words of the read (its
 * pieces), work[2 c + 1] = the same columns x (11 W + 8) -- the integer instructions per column and lane, i.e. what the kernel's
 * issue-rate roofline counts.  Measurement only (bench.py: prefilter_roofline); no reference counterpart. */
int clh_plan_prefilter_timing(clh_plan* pl, float* ms, int64_t* work);

/* Launch the batch on packed code arrays that already live in HBM (device pointers).  Asynchronous on `stream`
 * (a hipStream_t).  NULL selects the context's own, private, non-blocking stream -- NOT the legacy default stream: work
 * a caller has queued on the default stream (or on any other stream) is then unordered with these kernels.  A caller
 * who produces inputs or consumes clh_ssw_results_dev() on a stream of its own passes THAT stream; hipStreamLegacy /
 * hipStreamPerThread are passed through like any other handle.  Results stay in HBM until clh_ssw_fetch, which waits
 * for the stream of the last run.  The same holds for every `stream` argument of this header.
 * Matrix edge 6..32 with CIGARs wanted: d_reads and d_refs must stay allocated and unmodified until clh_ssw_fetch returns --
 * fetch may run tracebacks again (CLH_ST_CIGAR_TRUNC below) on the context's own stream, and they read both buffers. */
int clh_ssw_run(clh_plan* plan, const void* d_reads, const void* d_refs, void* stream);

/* Padding contract of d_refs.  For windows of 32 kb and more the column prefilter reads the window text in whole, address-aligned
 * 256-byte blocks: when d_refs is 256-byte aligned it may read up to 255 bytes past the last byte any window uses (never in front of
 * d_refs).  The buffer must be readable up to that boundary -- every hipMalloc / caching-allocator block is (allocations are rounded
 * to at least 256 bytes), a pointer INTO such a block that ends short of the boundary is not.  A caller who cannot promise it states the
 * buffer's size here (bytes from d_refs; -1 = unstated, the default): a run whose last block would cross it uses the static window
 * slices instead of the prefilter.  A d_refs that is not 256-byte aligned always does.  Results are the same either way. */
int clh_plan_set_refs_bytes(clh_plan* plan, int64_t nbytes);

/* Wait for the last run and copy results out.  cigar_buf may be NULL.  *cigar_used receives the u32 count (the CIGARs come back
 * as one dense array).  It waits for the completion of the plan's last clh_ssw_run (an event recorded behind its last launch),
 * not for work the caller queued on the stream afterwards.  Matrix edge 6..32 with CIGARs wanted: the tracebacks the run's shared
 * workspace could not hold are run here, on the context's own stream, over the emptied workspace (they read the run's d_reads and
 * d_refs, which must still hold the run's sequences), before the rows are read. */
int clh_ssw_fetch(clh_plan* plan, clh_align_t* out, uint32_t* cigar_buf, int64_t cigar_cap, int64_t* cigar_used);

/* Device pointer of the raw result table of the last run (8 x int32 per alignment: score1 score2 ref_begin1 ref_end1
 * read_begin1 read_end1 ref_end2 status), for callers that keep post-processing on the GPU.  Matrix edge 6..32: the CIGAR part of
 * `status` is final only after clh_ssw_fetch (before it, a row may carry an internal bit, 256, for a traceback still to run). */
const void* clh_ssw_results_dev(const clh_plan* plan);

/* Measurement hooks (bench.py): per launch-segment (one read-length class each) HIP-event durations of the score
 * kernel (K1), and of the traceback kernel (K1b): k1b_ms[0] = the small-window launch over all alignments,
 * k1b_ms[1] = the large-window launches that redo the outliers.  Both return the number of segments. */
int clh_plan_set_profiling(clh_plan* plan, int on);
int clh_plan_segments(const clh_plan* plan, int32_t cap, int32_t* rv, int32_t* count, int64_t* read_bases, int64_t* ref_bases);
int clh_plan_timing(clh_plan* plan, int32_t cap, float* k1_ms, float* k1b_ms);

/* Host-buffer convenience: plan + upload + run + fetch. */
int clh_ssw_batch(clh_ctx* ctx, int32_t n, const int8_t* reads, const int64_t* read_off, const int8_t* refs,
                  const int64_t* ref_off, const int32_t* mask_len, const clh_ssw_opts* opts,
                  clh_align_t* out, uint32_t* cigar_buf, int64_t cigar_cap, int64_t* cigar_used);

/* ---- cyclic consensus: the batch form of pyccs.find_consensus (CIRI_long/find_ccs.py:14) -----------------------
 * pyccs/spoa are external and absent from the reference tree (PARITY UNPINNED).  Per read: tandem-repeat period by
 * 8-mer self-matches and copy boundaries (this project's specification, oracle/ccs_oracle.c), then the consensus of
 * the copies by partial-order alignment as spoa computes it (oracle/poa_oracle.c: local alignment, scores
 * 10/-4/-8/-2/-24/-1 -- the call of the reference's tests/test_poa.py:30).  segs holds [start,end) pairs, 65 per read;
 * ccs is packed like reads. */
#define CLH_CCS_SEG_CAP 65
typedef struct {
    int32_t nseg;      /* 0: no tandem repeat / no consensus (find_consensus would return (None, None)) */
    int32_t ccs_len;
    int32_t period;
    int32_t status;    /* 0 ok; >0 no consensus because of a limit of this kernel (counted, see clh_ccs_plan_stats): 1 workspace, 2 graph limits (48
                          in-edges, 8 letters in a column, 65000 rows), 3 output, 4 sequence longer than 2800 bases, 5 back-track guard, 6 a DP
                          cell left the 16-bit range (global / overlap modes with costly gaps), 7 an alignment without a base (spoa throws) */
} clh_ccs_t;
typedef struct clh_ccs_plan clh_ccs_plan;
clh_ccs_plan* clh_ccs_plan_create(clh_ctx* ctx, int32_t n, const int64_t* read_off);
void clh_ccs_plan_destroy(clh_ccs_plan* plan);
int clh_ccs_run(clh_ccs_plan* plan, const void* d_reads, void* stream);
int clh_ccs_fetch(clh_ccs_plan* plan, clh_ccs_t* out, int32_t* segs, int8_t* ccs);
/* Device pointers of the last run's outputs (rows: clh_ccs_t[n]; segs: int32[n][2*65]; ccs: packed codes at the read
 * offsets), for callers that keep the next step on the GPU.  Any of the three may be NULL. */
int clh_ccs_results_dev(const clh_ccs_plan* plan, const void** rows, const void** segs, const void** ccs);
/* Workspace tiers of the plan and how the last run used them: out[6] = {first-tier slots, bytes per slot, large slots,
 * bytes per large slot, reads that ran in a large slot claimed on the fly, reads run by the second launch}. */
int clh_ccs_plan_info(clh_ccs_plan* plan, int64_t* out);
/* Work and losses of the last run: out[16] = {DP cells, DP row steps, alignments whose back-track left the band of cells the forward
 * pass had stored (run again with all cells: cost, never a different answer), reads that ended with status 1, 2, ... 7 (no
 * consensus because of a limit of this kernel -- never silently: callers count and report them), 0 ...}. */
int clh_ccs_plan_stats(clh_ccs_plan* plan, int64_t* out);
/* HIP-event durations (ms) of the last run: ms[0] = repeat scan (K2), ms[1] = partial-order consensus (K3). */
int clh_ccs_plan_timing(clh_ccs_plan* plan, float* ms);
int clh_ccs_batch(clh_ctx* ctx, int32_t n, const int8_t* reads, const int64_t* read_off, clh_ccs_t* out, int32_t* segs, int8_t* ccs);

/* The spoa.poa call shape -- poa(seqs, algorithm, genmsa, m, n, g, e, q, c), collapse.py:267,504 (algorithm 2),
 * tests/test_poa.py:30 (algorithm 0, genmsa) -- for a batch of groups of sequences.  Group k = sequences
 * [group_off[k], group_off[k+1]) of the packed array (any number >= 1, groups contiguous, each sequence <= 2800 bases).
 * opts NULL = {0, 10, -4, -8, -2, -24, -1, 0}.  algorithm: 0 local, 1 global, 2 overlap; a gap of k bases costs
 * max(g + (k-1) e, q + (k-1) c); g <= q or e >= c selects the one-piece (affine) model as spoa does; the linear model
 * (g >= e) and scores outside the kernel's 16-bit cells (m 1..11, e - g <= 6, c - q <= 30) fail with CLH_E_UNSUPPORTED --
 * nothing is silently ignored.  min_coverage > 0 leaves nodes crossed by fewer sequences out of the consensus.
 * out_ccs is packed by the offset of each group's first sequence; out_len[k] < 0 when no consensus could be built
 * (-(1 + status), status as in clh_ccs_t).  msa_col (may be NULL; one int32 per base, packed like seqs) receives the MSA
 * column of every base, msa_ncols[k] the number of columns of group k: row i of the MSA is '-' everywhere except
 * row[msa_col[b]] = base b for the bases b of sequence i.  aln_score (may be NULL; int32[ngroups][65]) receives the
 * end-cell score of the alignment of each of the first 65 sequences of a group. */
typedef struct { int32_t algorithm, m, n, g, e, q, c, min_coverage; } clh_poa_opts;
/* clh_ccs_plan_stats of the last clh_poa_batch of this context (out[16], same layout) */
int clh_poa_last_stats(clh_ctx* ctx, int64_t* out);
int clh_poa_batch(clh_ctx* ctx, int32_t ngroups, const int8_t* seqs, const int64_t* seq_off, const int64_t* group_off,
                  const clh_poa_opts* opts, int32_t* out_len, int8_t* out_ccs, int32_t* msa_col, int32_t* msa_ncols, int32_t* aln_score);

/* ---- Stage 1 from file to file -------------------------------------------------------------
 * The read loop of find_ccs_reads (CIRI_long/find_ccs.py:29-96) in native code: FASTA/FASTQ, plain or gzip, one header and
 * one sequence line per record; writes tmp/{prefix}.ccs.fa and tmp/{prefix}.raw.fa in the reference's format
 * (find_ccs.py:94-95), reads with a consensus only, input order.  batch_reads <= 0 selects 65536.  too_long counts reads
 * above 16 M bases (not scanned). */
typedef struct { int64_t total_reads, ro_reads, too_long, capacity_dropped; } clh_ccs_file_stats;   /* capacity_dropped: reads with a
                                                                   tandem repeat that a limit of the kernel left without a consensus (status > 0) */
int clh_ccs_file(clh_ctx* ctx, const char* in_path, int is_fastq, const char* ccs_fa_path, const char* raw_fa_path,
                 int32_t batch_reads, clh_ccs_file_stats* stats);
/* The same for the records [first_record, first_record + max_records) of the file (max_records < 0: to the end) -- one
 * rank's contiguous shard of the reads (the reference hands chunks of the record stream to its pool, find_ccs.py:66-75);
 * concatenating the outputs of consecutive shards gives the files of the unsharded call, byte for byte. */
int clh_ccs_file_range(clh_ctx* ctx, const char* in_path, int is_fastq, const char* ccs_fa_path, const char* raw_fa_path,
                       int32_t batch_reads, int64_t first_record, int64_t max_records, clh_ccs_file_stats* stats);
/* number of records of a FASTA/FASTQ(.gz) file as that loop counts them (host only) */
int clh_fastx_count(const char* in_path, int is_fastq, int64_t* n_records);
/* the same count plus the byte offset of every `every`-th record (0, every, 2 every ...; at most `cap`) of an uncompressed file
 * (*n_offsets = 0 for a gzip file), and stage 1 for the records [first_record, first_record + max_records) counted from such an
 * offset: a rank of a sharded `call` (the reference hands chunks of the record stream to its pool, find_ccs.py:66-75) seeks to its
 * shard instead of reading past what lies in front of it (host I/O only; find_ccs.py:29-64 for what a record is) */
int clh_fastx_index(const char* in_path, int is_fastq, int64_t every, int64_t* n_records, int64_t* offsets, int64_t cap, int64_t* n_offsets);
int clh_ccs_file_at(clh_ctx* ctx, const char* in_path, int is_fastq, const char* ccs_fa_path, const char* raw_fa_path,
                    int32_t batch_reads, int64_t byte_offset, int64_t first_record, int64_t max_records, clh_ccs_file_stats* stats);
/* The file stage keeps its host buffers (six batches of file text and base codes, ~70 MB each) and two device buffers between calls,
 * one set per process; this gives them back. */
void clh_ccs_file_release_buffers(void);

/* ---- Resident genome ---------------------------------------------------------------------
 * The reference builds, per clipped read, a window string of hit +- 200 kb, counts its 'N', reverse-complements it for
 * minus-strand hits and encodes it base by base in Python (CIRI_long/find_bsj.py:196-201,214;
 * libs/striped_smith_waterman/ssw_wrap.py:234-252).  Here the genome (all contigs concatenated by the caller, who keeps
 * the contig offsets) is encoded once into HBM and a window is (offset, length, strand): clh_ssw_plan_windows +
 * clh_ssw_run(plan, d_reads, clh_genome_codes(genome), stream) give the results clh_ssw_plan/clh_ssw_run give for the
 * window strings built the reference's way -- including its handling of lower-case bases (reversed, not complemented). */
typedef struct clh_genome clh_genome;
clh_genome* clh_genome_create(clh_ctx* ctx, const char* ascii, int64_t len);
void clh_genome_destroy(clh_genome* genome);
const void* clh_genome_codes(const clh_genome* genome);      /* device pointer */
int64_t clh_genome_length(const clh_genome* genome);
/* out[k] = number of upper-case 'N' in [off[k], off[k]+len[k]) -- Counter(window)['N'] of find_bsj.py:199 */
int clh_genome_count_n(clh_genome* genome, int32_t n, const int64_t* off, const int64_t* len, int64_t* out);
/* the letters of the spans [off[k], off[k]+len[k]) as codes 0..4 (bits 0-2 of the resident byte, clamped to 4), packed one span behind
 * the other into out: one gather on the device (one lane a span, so meant for short spans such as the dinucleotides beside refined
 * junctions, many of them at once) and one copy back.  CLH_E_ARG: a span outside the genome. */
int clh_genome_letters(clh_genome* genome, int32_t n, const int64_t* off, const int64_t* len, int8_t* out);
/* Annotated splice sites for clh_splice_signal_batch: the reference's splice_site_index / circ_ss_idx
 * (CIRI_long/align.py:235-252, 275-316: index[contig][pos][strand]['start'|'end']) flattened to four runs of genome-wide
 * positions (contig offset in the resident genome + pos), each strictly ascending, concatenated in `pos` in the order
 * '+' starts, '+' ends, '-' starts, '-' ends; count4 = their lengths.  Replaces any earlier set; all zero = none. */
int clh_genome_set_splice_sites(clh_genome* genome, const int64_t* pos, const int64_t* count4);
/* Splice signals around n candidate back-splice junctions [start, end) (0-based) of contigs of the resident genome --
 * CIRI_long/align.py:477-493 (free sliding), :495-568 (pairs of annotated sites, if sites were set), :571-695
 * (find_denovo_signal, annotated shifts joining the motif occurrences) and :698-733 (ranking), as called from
 * find_bsj.py:286-301 with search_length = clip_base + search_extra (10), shift_threshold (3).
 * host_mask: strands of the host gene, bit 0 '+', bit 1 '-'.  out[8k..8k+7] = status (0 done, 1 = outside this kernel's
 * domain: the neighbourhood leaves the contig or holds non-ACGTN characters; run the Python statement), us_free,
 * ds_free, found (0 none, 1 de novo, 2 annotated pair), strand (0 '+', 1 '-'), us_shift, ds_shift, motif (de novo:
 * index into GT-AG, GC-AG, AT-AC, GT-AC, AT-AG).
 * is_canonical: bit 0 = search GT-AG only; bit 1 = the two search windows are cut the way a minimap2 index serves sequences
 * (mappy.Aligner.seq, env.GENOME of the reference's main pass, find_bsj.py:340-341: no sequence for a start outside the contig,
 * end clipped) instead of the way Python slices a string (align.Fasta.seq, the short-read pass, find_bsj.py:455,462).
 * CLH_E_ARG for clip_base outside [0, 4096], a negative search_extra or shift_threshold, and clip_base + search_extra above
 * 16284 (the ranking key keeps 15 bits per component).  With annotated sites set, a candidate away from the contig ends whose
 * 2 (clip_base + search_extra) exceeds 64 gets status 1 as well. */
int clh_splice_signal_batch(clh_genome* genome, int32_t n, const int64_t* ctg_off, const int64_t* ctg_len, const int64_t* start,
                            const int64_t* end, const int32_t* clip_base, const int32_t* host_mask, int32_t search_extra,
                            int32_t shift_threshold, int32_t is_canonical, int32_t* out);
/* like clh_ssw_plan, references given as windows of the resident genome; win_rc[k] != 0: minus strand */
clh_plan* clh_ssw_plan_windows(clh_ctx* ctx, int32_t n, const int64_t* read_off, const int64_t* win_off, const int32_t* win_len,
                               const uint8_t* win_rc, const int32_t* mask_len, const clh_ssw_opts* opts);

/* one call: reads from the host, references = windows of the resident genome (same outputs as clh_ssw_batch) */
int clh_ssw_windows_batch(clh_genome* genome, int32_t n, const int8_t* reads, const int64_t* read_off, const int64_t* win_off,
                          const int32_t* win_len, const uint8_t* win_rc, const int32_t* mask_len, const clh_ssw_opts* opts,
                          clh_align_t* out, uint32_t* cigar_buf, int64_t cigar_cap, int64_t* cigar_used);

/* Unit-cost edit distance of n pairs of byte strings: what the reference's distance(x, y) returns (CIRI_long/utils.py:
 * 153-159; python-Levenshtein for <= 50 characters, edlib otherwise -- the same integer), used pairwise by
 * cluster_sequence (collapse.py:466-473) and per candidate by avg_score (collapse.py:156-158).  Strings are compared
 * byte for byte (case-sensitive, like the reference); pair k is a[a_off[k]..a_off[k+1]) against b[b_off[k]..b_off[k+1]).
 * No length limit (a shorter string above 4096 bytes is swept in passes). */
int clh_edit_distance_batch(clh_ctx* ctx, int32_t n, const uint8_t* a, const int64_t* a_off, const uint8_t* b, const int64_t* b_off,
                            int32_t* out);

/* the same in three steps, for batches that stay resident (strings uploaded once, any number of runs) */
typedef struct clh_edit_plan clh_edit_plan;
clh_edit_plan* clh_edit_plan_create(clh_ctx* ctx, int32_t n, const uint8_t* a, const int64_t* a_off, const uint8_t* b, const int64_t* b_off);
void clh_edit_plan_destroy(clh_edit_plan* plan);
int clh_edit_plan_run(clh_edit_plan* plan, void* stream);
int clh_edit_plan_fetch(clh_edit_plan* plan, int32_t* out);
int clh_edit_plan_timing(clh_edit_plan* plan, float* ms);       /* HIP-event duration of the last run */

/* ---- edit-distance matrices of whole groups ----------------------------------------------------------------------------
 * The distance matrix cluster_sequence builds (collapse.py:466-473), for many lists at once, without writing the pairs
 * out: string s is seqs[seq_off[s]..seq_off[s+1]) (nseq strings, uploaded once), group g is the strings group_off[g] ..
 * group_off[g+1]-1 (ngroups groups; 0 <= group_off[0], ascending, group_off[ngroups] <= nseq).  A group of m strings
 * yields its m(m-1)/2 distances i < j in the order of the condensed upper triangle (row by row: scipy's pdist order);
 * dist is the groups' triangles one after the other.  With CLH_EM_HPC every string is homopolymer-compressed on the
 * device first (utils.py:162-167: each run of equal bytes becomes one) and the distances are those of the compressed
 * strings.  len[s]: the length string s was compared at; hpc (may be NULL): the compressed strings, dense, in string
 * order (the strings as given without CLH_EM_HPC).  Strings outside every group are compressed and not compared, so
 * ngroups = 0 is the compression alone.
 * create fails with CLH_E_ARG for offsets that do not ascend or a string of 2^31 bytes or more, and with CLH_E_CAPACITY
 * for more than 2^31 - 1 pairs in all; fetch with CLH_E_CAPACITY when dist_cap (int32 entries) or hpc_cap (bytes) is
 * too small.  stream NULL = libclh's private stream.  sizes: hpc_bytes is known once the plan has run. */
#define CLH_EM_HPC 1     /* homopolymer-compress every string on the device first */
typedef struct clh_edit_matrix_plan clh_edit_matrix_plan;
clh_edit_matrix_plan* clh_edit_matrix_plan_create(clh_ctx* ctx, int32_t nseq, const uint8_t* seqs, const int64_t* seq_off, int32_t ngroups,
                                                  const int64_t* group_off, int32_t flags);
void clh_edit_matrix_plan_destroy(clh_edit_matrix_plan* plan);
int clh_edit_matrix_plan_run(clh_edit_matrix_plan* plan, void* stream);
int clh_edit_matrix_plan_sizes(clh_edit_matrix_plan* plan, int64_t* npairs, int64_t* hpc_bytes);
int clh_edit_matrix_plan_fetch(clh_edit_matrix_plan* plan, int32_t* dist, int64_t dist_cap, int32_t* len, uint8_t* hpc, int64_t hpc_cap);
int clh_edit_matrix_plan_timing(clh_edit_matrix_plan* plan, float* ms);     /* HIP events around the last run: compression, task build, K4 */
/* create + run + fetch */
int clh_edit_matrix_batch(clh_ctx* ctx, int32_t nseq, const uint8_t* seqs, const int64_t* seq_off, int32_t ngroups, const int64_t* group_off,
                          int32_t flags, int32_t* dist, int64_t dist_cap, int32_t* len, uint8_t* hpc, int64_t hpc_cap);

/* ---- edlib.align: modes, end / start locations, CIGARs ----------------------------------------------------------------
 * Unit-cost alignment of the whole query (pattern) q[q_off[k]..q_off[k+1]) against the target t[t_off[k]..t_off[k+1]),
 * bytes compared for equality (any byte value).  mode: CLH_EA_NW (whole target), CLH_EA_SHW (a prefix of the target),
 * CLH_EA_HW (any substring).  task: CLH_EA_DISTANCE (distance and end locations), CLH_EA_LOCATIONS (+ starts),
 * CLH_EA_PATH (+ the CIGAR of the first location).  k >= 0: a best above k gives distance -1, no location, no CIGAR
 * (status CLH_EA_ST_ABOVE_K).  eq: n_eq pairs of letters (2 n_eq bytes) that also count as equal (symmetric, not
 * transitive).  workspace_bytes: the path pass's storage per chunk of the batch (0: 1 GiB); a pair that alone needs more
 * fails with CLH_E_CAPACITY.
 * Row k: distance, nlocs locations at locs[2 loc_off ..] as (start, end) int32 pairs, both inclusive, 0-based; end -1 =
 * before the first target letter; start -1 = not computed (task distance).  The CIGAR (task path) is cigar_len BAM-style
 * uint32 ops (len << 4 | op; = 7, X 8, I 1 query letter, D 2 target letter) at cigar[cigar_off ..].  alphabet_len: the
 * number of distinct bytes in query and target.  locs_cap is counted in locations, cigar_cap in ops. */
#define CLH_EA_NW  0
#define CLH_EA_SHW 1
#define CLH_EA_HW  2
#define CLH_EA_DISTANCE  0
#define CLH_EA_LOCATIONS 1
#define CLH_EA_PATH      2
#define CLH_EA_ST_ABOVE_K 1
typedef struct { int32_t mode, task, k, n_eq; const uint8_t* eq; int64_t workspace_bytes; } clh_edit_align_opts;
typedef struct { int32_t distance, nlocs; int64_t loc_off, cigar_off; int32_t cigar_len, status, alphabet_len, reserved; } clh_edit_align_row;
int clh_edit_align_batch(clh_ctx* ctx, int32_t n, const uint8_t* q, const int64_t* q_off, const uint8_t* t, const int64_t* t_off,
                         const clh_edit_align_opts* opts, clh_edit_align_row* rows, int32_t* locs, int64_t locs_cap, int64_t* locs_used,
                         uint32_t* cigar, int64_t cigar_cap, int64_t* cigar_used);
/* the same in three steps (strings uploaded once, any number of runs; a timed run excludes the upload) */
typedef struct clh_edit_align_plan clh_edit_align_plan;
clh_edit_align_plan* clh_edit_align_plan_create(clh_ctx* ctx, int32_t n, const uint8_t* q, const int64_t* q_off, const uint8_t* t,
                                                const int64_t* t_off, const clh_edit_align_opts* opts);
void clh_edit_align_plan_destroy(clh_edit_align_plan* plan);
int clh_edit_align_plan_run(clh_edit_align_plan* plan, void* stream);
int clh_edit_align_plan_fetch(clh_edit_align_plan* plan, clh_edit_align_row* rows, int32_t* locs, int64_t locs_cap, int64_t* locs_used,
                              uint32_t* cigar, int64_t cigar_cap, int64_t* cigar_used);
int clh_edit_align_plan_timing(clh_edit_align_plan* plan, float* ms);   /* HIP-event duration of the last run */
/* capacities fetch needs for this plan: locations and CIGAR ops */
int clh_edit_align_plan_caps(clh_edit_align_plan* plan, int64_t* locs_cap, int64_t* cigar_cap);

/* ---- edlib.search: short probes against whole sets of texts ---------------------------------------------------------------
 * The cross product the adapter, primer and junction-probe searches want, without writing it out: every probe
 * probes[probe_off[p]..probe_off[p+1]) (at most 64 letters) against every text texts[text_off[t]..text_off[t+1]), both
 * uploaded once.  Cell (t, p) is row t * nprobe + p and holds what clh_edit_align_batch returns for that pair with mode
 * CLH_EA_HW and task CLH_EA_LOCATIONS: distance, (start, end) of the first location, the end of the last location and the
 * number of locations (the tie rules of that call: column -1 is a candidate, the start is the longest alignment's).  Without a
 * location (k >= 0 and a best above k: distance -1, nlocs 0) start, end and last_end are -2.  eq: n_eq pairs of letters (2 n_eq
 * bytes) that also count as equal, symmetric, not transitive, applied to the letters as given.  Strands are the caller's
 * business: a search on both strands passes each probe and its reverse complement.
 * One wave takes one cell and its 64 lanes walk 64 column segments of the text at once (csrc/edit_search.hip); info reports the
 * geometry: out[8] = {columns a lane owns per round (SEG), columns of a wave's round (64 SEG), columns one wave walks before a
 * text is split over several waves, texts per launch (all of them: launches are not split), chunks of all texts, texts split
 * over more than one wave, probes of 1..32 letters (32-bit words), probes of 33..64 letters}.
 * create fails with CLH_E_ARG for offsets that do not ascend, a probe above 64 letters or a text above 2^30 bytes; fetch with
 * CLH_E_CAPACITY when rows_cap (records) is below ntext * nprobe, and with CLH_E_HIP if a kernel left a cell unwritten (never a
 * value).  Life cycle, error codes and `stream` as clh_edit_matrix_plan_*. */
typedef struct { int32_t k, n_eq; const uint8_t* eq; } clh_edit_search_opts;
typedef struct { int32_t distance, start, end, last_end, nlocs; } clh_edit_search_row;
typedef struct clh_edit_search_plan clh_edit_search_plan;
clh_edit_search_plan* clh_edit_search_plan_create(clh_ctx* ctx, int32_t ntext, const uint8_t* texts, const int64_t* text_off, int32_t nprobe,
                                                  const uint8_t* probes, const int64_t* probe_off, const clh_edit_search_opts* opts);
void clh_edit_search_plan_destroy(clh_edit_search_plan* plan);
int clh_edit_search_plan_run(clh_edit_search_plan* plan, void* stream);
int clh_edit_search_plan_fetch(clh_edit_search_plan* plan, clh_edit_search_row* rows, int64_t rows_cap);
int clh_edit_search_plan_timing(clh_edit_search_plan* plan, float* ms);     /* HIP events around the last run */
int clh_edit_search_plan_info(clh_edit_search_plan* plan, int64_t* out);
/* create + run + fetch */
int clh_edit_search_batch(clh_ctx* ctx, int32_t ntext, const uint8_t* texts, const int64_t* text_off, int32_t nprobe, const uint8_t* probes,
                          const int64_t* probe_off, const clh_edit_search_opts* opts, clh_edit_search_row* rows, int64_t rows_cap);

/* ---- end-anchored affine-gap alignment of pairs: global, semiglobal, overlap (K1g) ------------------------------------------
 * What clh_ssw_* does locally, anchored at the ends: query q[q_off[k]..q_off[k+1]) against reference r[r_off[k]..r_off[k+1]), both as
 * codes in [0, n_mat), under the substitution matrix `mat` (n_mat x n_mat, row = reference code, as in clh_ssw_opts) and a gap of
 * k letters costing gap_open + (k - 1) gap_extend.  With cells (i, j), i query letters against j reference letters:
 *     E[i][j] = max(H[i][j-1] - go, E[i][j-1] - ge)   (CIGAR D)      F[i][j] = max(H[i-1][j] - go, F[i-1][j] - ge)   (CIGAR I)
 *     H[i][j] = max(H[i-1][j-1] + s(q[i-1], r[j-1]), E[i][j], F[i][j]),   H[0][0] = 0
 * CLH_ENDS_GLOBAL: row 0 and column 0 are one gap, the end cell is (m, n).  CLH_ENDS_SEMIGLOBAL (the whole query in any stretch of
 * the reference): row 0 is 0, column 0 one gap, the end cell is the greatest H[m][j], smallest j.  CLH_ENDS_OVERLAP (end gaps free on
 * both sequences at both ends): row 0 and column 0 are 0, the end cell is the greatest H of the last row and the last column,
 * last-row cells first, smallest j, then smallest i.  The walk back prefers the diagonal, then E, then F, leaves a gap as soon as
 * E[i][j] == H[i][j-1] - go (F likewise), takes the remaining letters of a boundary that is not free as one gap, and stops at (0, 0)
 * (global), on row 0 (semiglobal, overlap) or column 0 (overlap).  DESIGN.md section 6 has the rules in full; parity with other
 * libraries is unpinned.
 * Start-anchored (pinned at (0, 0), free at the far end; what seed-and-extend needs): row 0, column 0 and the walk are global's,
 * ref_begin = query_begin = 0, the walk stops at (0, 0), letters beyond the end cell are not part of the CIGAR.  CLH_ENDS_PREFIX
 * (the whole query against a prefix of the reference): the end cell is the greatest H[m][j], 0 <= j <= n, smallest j; at (0, 1, 1, 1)
 * the score is minus edlib's SHW distance and ref_end its first end location.  CLH_ENDS_EXTEND (a prefix of the query against a
 * prefix of the reference): the end cell is the greatest H[i][j] over all cells, (0, 0) with H = 0 included, smallest i, then
 * smallest j; the score is >= 0 and the empty result has ref_end = query_end = -1 and no CIGAR.  Neither is a z-drop or X-drop
 * heuristic: both are defined by the full matrix.  An empty side: extend 0 and empty; prefix 0 and empty without a query letter,
 * -(go + (m - 1) ge) and mI without a reference letter.  Parity with ksw2's extension and parasail is unpinned and not claimed.
 * Row k: score (int32, may be negative); ref / query begin and end, 0-based and inclusive as in clh_align_t, end == begin - 1 for a
 * span without a letter; with want_cigar the CIGAR as cigar_len packed ops (len << 4 | op; M 0, I 1, D 2 as clh_ssw_fetch returns
 * them, M for match and mismatch, free end gaps not part of it) at cigar[cigar_off ..].  Without want_cigar no walk is made:
 * cigar_off is -1 and a begin the mode does not fix (ref_begin outside global, query_begin in overlap) is -1.
 * create fails with CLH_E_UNSUPPORTED for gap_open < gap_extend; with CLH_E_ARG for a code outside the matrix (the message names
 * the first such pair) and for a pair with (m + n) max(|s|, gap_open, gap_extend) >= 2^30 (the cells are int32); with
 * CLH_E_CAPACITY when the stored decisions of one pair (half a byte per cell) exceed workspace_bytes (0: 1 GiB) -- a batch is cut
 * into shares that fit it.  A pair with an empty side never reaches a kernel; fetch states the programme's answer.  fetch fails
 * with CLH_E_CAPACITY when cigar_cap (ops) is too small -- info's out[7] always suffices -- and with CLH_E_HIP if a kernel left a row
 * unwritten (never a value).  info: out[8] = {columns a lane owns, columns of a chunk (a longer reference is walked chunk after
 * chunk), shares of the batch, workspace bytes in use, those of the largest pair, pairs the kernels take, pairs with an empty side,
 * CIGAR ops fetch may return}.  Life cycle, error codes and `stream` as clh_edit_align_plan_*.
 * want_cigar: 0 no CIGARs; 1 (and any other non-zero value) the stored route described above; CLH_ENDS_CIGAR_RECOMPUTE (2) the
 * recompute route, for clh_ends_plan_create, _gap2 and _spliced and their _batch forms alike.  Rows and CIGARs are bit for bit the
 * stored route's; what differs is the workspace.  The score pass keeps the last column of every chunk of 512 columns but the last, the
 * decisions are computed again one chunk at a time, for the rows the walk can still reach, and the walk is resumed chunk after chunk
 * leftwards.  With mpad = (m + 63) & ~63, nchunks = ceil(n / 512), NH = 2 (one piece) or 3 (two pieces, spliced) and W = 4 (one
 * piece) or 8 bytes, a pair needs
 *     4 NH mpad (nchunks - 1)  kept columns  +  W m 64  one chunk's plane  +  48  the walk's resume record,   rounded up to 16,
 * where the stored route needs W m (64 (nchunks - 1) + lanes of the last chunk).  That sum is what is held against workspace_bytes
 * -- CLH_E_CAPACITY names it for a pair that exceeds it alone -- what the shares are cut by and what info's out[2..4] report.
 * Below about four chunks it saves little, and it computes every cell the walk can reach a second time: the choice is the caller's,
 * no routing is made.  clh_band_* has no such route: there every non-zero want_cigar is the stored route. */
#define CLH_ENDS_CIGAR_STORED    1
#define CLH_ENDS_CIGAR_RECOMPUTE 2
#define CLH_ENDS_GLOBAL     0
#define CLH_ENDS_SEMIGLOBAL 1
#define CLH_ENDS_OVERLAP    2
#define CLH_ENDS_PREFIX     3
#define CLH_ENDS_EXTEND     4
typedef struct { int32_t mode; const int8_t* mat; int32_t n_mat; int32_t gap_open, gap_extend; int32_t want_cigar; int64_t workspace_bytes; } clh_ends_opts;
typedef struct { int32_t score, ref_begin, ref_end, query_begin, query_end, cigar_len; int64_t cigar_off; } clh_ends_row;
typedef struct clh_ends_plan clh_ends_plan;
clh_ends_plan* clh_ends_plan_create(clh_ctx* ctx, int32_t n, const int8_t* q, const int64_t* q_off, const int8_t* r, const int64_t* r_off,
                                    const clh_ends_opts* opts);
void clh_ends_plan_destroy(clh_ends_plan* plan);
int clh_ends_plan_run(clh_ends_plan* plan, void* stream);
int clh_ends_plan_fetch(clh_ends_plan* plan, clh_ends_row* rows, uint32_t* cigar, int64_t cigar_cap, int64_t* cigar_used);
int clh_ends_plan_timing(clh_ends_plan* plan, float* ms);     /* HIP events around the last run */
int clh_ends_plan_info(clh_ends_plan* plan, int64_t* out);
/* create + run + fetch */
int clh_ends_batch(clh_ctx* ctx, int32_t n, const int8_t* q, const int64_t* q_off, const int8_t* r, const int64_t* r_off, const clh_ends_opts* opts,
                   clh_ends_row* rows, uint32_t* cigar, int64_t cigar_cap, int64_t* cigar_used);

/* Two-piece gap costs for clh_ends_*: with gap2 a gap of k letters costs min(gap_open + (k - 1) gap_extend, gap_open2 + (k - 1)
 * gap_extend2) -- piece 1 (the fields of clh_ends_opts) for short gaps, piece 2 for long ones.  Each direction has one state per piece,
 *     E_p[i][j] = max(H[i][j-1] - go_p, E_p[i][j-1] - ge_p)      F_p[i][j] = max(H[i-1][j] - go_p, F_p[i-1][j] - ge_p)      p = 1, 2
 *     H[i][j]   = max(H[i-1][j-1] + s, E_1, E_2, F_1, F_2)
 * Modes, boundaries (a boundary gap of j letters costs the smaller piece), end cells, coordinates, empty sides and CIGAR conventions
 * are those of clh_ends_*.  The walk prefers the diagonal, then E_1, E_2, F_1, F_2, and leaves E_p as soon as E_p[i][j] == H[i][j-1] -
 * go_p (F_p likewise); both pieces emit the same op.  Admitted: 0 <= gap_extend2 <= gap_extend <= gap_open <= gap_open2 (equal pieces
 * included), anything else is CLH_E_UNSUPPORTED and the message names the inequality; under these a maximal run of D or I is never
 * cheaper split over both pieces, so the score is the best over all alignments with every run costed by the minimum.  The range
 * bound takes the maximum over all four costs.  Stored decisions are one byte per cell, twice the one-piece figure: CLH_E_CAPACITY,
 * the shares and info's byte counts follow.  The plan is a clh_ends_plan: run, fetch, timing, info and destroy are those above.
 * gap2 == NULL is clh_ends_plan_create / clh_ends_batch.  clh_band_*_gap2 below are the same costs over a band. */
typedef struct { int32_t gap_open2, gap_extend2; } clh_gap2;
clh_ends_plan* clh_ends_plan_create_gap2(clh_ctx* ctx, int32_t n, const int8_t* q, const int64_t* q_off, const int8_t* r, const int64_t* r_off,
                                         const clh_ends_opts* opts, const clh_gap2* gap2);
int clh_ends_batch_gap2(clh_ctx* ctx, int32_t n, const int8_t* q, const int64_t* q_off, const int8_t* r, const int64_t* r_off, const clh_ends_opts* opts,
                        const clh_gap2* gap2, clh_ends_row* rows, uint32_t* cigar, int64_t cigar_cap, int64_t* cigar_used);

/* Spliced alignment for clh_ends_*: a long reference gap may be an intron, which costs a constant that depends on the dinucleotides at
 * its two ends and not on its length.  Sequences are DNA codes A, C, G, T = 0..3, anything else 4; the matrix must be the 5 x 5 match /
 * mismatch one (0 against code 4).  donor[4 a + b] and acceptor[4 a + b] are the costs of the dinucleotide (a, b) as read on the
 * transcript strand, `other` that of a dinucleotide which holds a code >= 4 or runs off the reference; strand[k] is +1 or -1 (strand
 * == NULL: all +1).  One rule: a maximal run of skipped reference letters r[a..b] (0-based, no query letter consumed in between) costs
 *     min(gap_open + (b - a) gap_extend, intron_open + start(a) + end(b));                          insertions are unchanged
 *     strand +:  start(a) = donor[r[a], r[a+1]]               end(b) = acceptor[r[b-1], r[b]]
 *     strand -:  start(a) = acceptor[c(r[a+1]), c(r[a])]      end(b) = donor[c(r[b]), c(r[b-1])]      c(x) = 3 - x
 * (a canonical intron reads CT..AC on the reference for strand -); a + 1 > n - 1 or b - 1 < 0 gives `other`.  The costs depend on the
 * position alone: for a run of one letter the second letter of the start dinucleotide lies outside the run.  In cells, 1-based
 * columns, don(j) = start(j - 1), acc(j) = end(j - 1):
 *     F[i][j] = max(H[i-1][j] - go, F[i-1][j] - ge)            (I; reads the true H)
 *     T[i][j] = max(H[i-1][j-1] + s(q_i, r_j), F[i][j])        (H without a reference gap)
 *     E[i][j] = max(T[i][j-1] - go, E[i][j-1] - ge)            (D)
 *     N[i][j] = max(T[i][j-1] - io - don(j), N[i][j-1])        (N; the close cost is paid on leaving)
 *     H[i][j] = max(T[i][j], E[i][j], N[i][j] - acc(j))
 * E and N open from T, not from H: a deletion run and an intron run are never adjacent, which makes the one rule exact; inserted
 * letters may separate them (D, I, N).  Modes, boundaries, end cells, coordinates and empty sides are those of clh_ends_*; row 0 of the
 * anchored modes is what the recurrences give from T[0][0] = 0, H[0][j] = -min(go + (j - 1) ge, io + don(1) + acc(j)); column 0 is
 * unchanged.  The walk prefers, in state H, the diagonal, then E, then N, then F; in state E it emits D, moves left and leaves as soon
 * as E[i][j] == T[i][j-1] - go, N likewise with N[i][j] == T[i][j-1] - io - don(j), emitting BAM op N (3); on leaving E or N it is in
 * state T: the diagonal if T equals it, else F.  The anchored stop on row 0 at column j > 0 emits one run of j letters, D if the
 * deletion is not dearer, else N: the CIGAR says which piece paid.  All costs must be >= 0 (CLH_E_ARG); a matrix of another form is
 * CLH_E_UNSUPPORTED; the range bound is (m + n) max(|s|, gap_open, gap_extend, intron_open + dmax + amax) < 2^30 with dmax, amax the
 * greatest donor and acceptor cost, `other` included.  Stored decisions are one byte per cell, the two-piece figure: CLH_E_CAPACITY,
 * the shares and info's byte counts follow.  The plan is a clh_ends_plan: run, fetch, timing, info and destroy are those above.
 * Two-piece gap costs together with introns, a band, and coupled donor-acceptor scoring are not built; parity with minimap2's splice
 * model, which couples the two sites and has other tie rules, is not claimed. */
typedef struct { int32_t intron_open; int32_t donor[16]; int32_t acceptor[16]; int32_t other; } clh_splice;
clh_ends_plan* clh_ends_plan_create_spliced(clh_ctx* ctx, int32_t n, const int8_t* q, const int64_t* q_off, const int8_t* r, const int64_t* r_off,
                                            const clh_ends_opts* opts, const clh_splice* splice, const int8_t* strand);
int clh_ends_batch_spliced(clh_ctx* ctx, int32_t n, const int8_t* q, const int64_t* q_off, const int8_t* r, const int64_t* r_off, const clh_ends_opts* opts,
                           const clh_splice* splice, const int8_t* strand, clh_ends_row* rows, uint32_t* cigar, int64_t cigar_cap, int64_t* cigar_used);

/* ---- banded end-anchored alignment of pairs around a diagonal: global, semiglobal, prefix, extend (K1gb) ---------------------------
 * The programme of clh_ends_* over a band.  The band of pair k is a closed interval of diagonals [lo, hi], d = j - i: without a hint
 * (diag == NULL) lo = min(0, n - m) - band, hi = max(0, n - m) + band; with diag[k], lo = diag[k] - band, hi = diag[k] + band; both
 * are then clipped to [-m, n], and everything below is about the clipped band.  Every cell outside the band is minus infinity in H, E
 * and F, and row 0 and column 0 come from the same recurrences, started at (0, 0), not from a formula: so every score is the score
 * of an alignment all of whose cells lie in the band.  CLH_ENDS_GLOBAL: H[0][j] = E[0][j] is the gap of j letters where the band
 * holds it, column 0 likewise through F, the end cell is (m, n).  CLH_ENDS_SEMIGLOBAL: row 0 is 0 on the band's cells, column 0 is
 * reached only while (0, 0) and the cells below it are in the band, the end cell is the greatest H[m][j] over the band's cells of
 * row m, smallest j.  The walk back is that of clh_ends_*; a source outside the band is no source.
 * create fails -- each message names the first such pair -- with CLH_E_ARG for a global band that misses (0, 0) or (m, n), lo >
 * min(0, n - m) or hi < max(0, n - m); with CLH_E_ARG for a semiglobal band with hi < 0 (no start cell) or lo > n - m (no end cell).
 * These conditions guarantee a path inside the band.  Global: the band holds every diagonal between 0 and n - m, so the gap from (0,
 * 0) to diagonal n - m, then that diagonal to (m, n), lies in it.  Semiglobal: d = min(hi, n - m) is a diagonal of the band, since lo
 * <= hi and lo <= n - m.  If d >= 0 the cells (0, d) .. (m, m + d) exist (m + d <= n) and are a path.  If d < 0 then d = n - m, as hi
 * >= 0; the band holds the diagonals d .. 0, and column 0 from (0, 0) down to (-d, 0), then diagonal d to (m, n), is a path.  By the
 * same steps every cell of such a band is reached from a start cell, which is what lets the kernel tell scores from minus
 * infinity.  Further refusals: CLH_E_UNSUPPORTED for CLH_ENDS_OVERLAP (a banded overlap is not built) and for gap_open < gap_extend;
 * CLH_E_CAPACITY for a clipped band of more than 512 diagonals (clh_ends_* takes such pairs over the full matrix) and for one pair
 * whose stored decisions -- half a byte per cell of the band, m ceil(B / CPL) CPL / 2 bytes -- exceed workspace_bytes (0: 1 GiB);
 * CLH_E_ARG for a code outside the matrix and for a pair with (m + n + 1024) max(|s|, gap_open, gap_extend, 1) >= 2^29: the cells
 * are int32 and minus infinity is -2^30, so every score, also moved into the scan's frame (+ at most 512 gap_extend), stays inside
 * (-2^29, 2^29) while anything derived from minus infinity stays below -2^29 and above INT32_MIN.
 * Row k: the fields of clh_ends_row, the clipped band, and `exact`: 1 means it is proved that clh_ends_* returns the same row and
 * the same CIGAR, 0 that it is not proved (they may still be equal).  A global alignment that leaves the band reaches diagonal hi +
 * 1 or lo - 1 and therefore has two gap runs of known least lengths and a bounded number of M columns; with s+ = max(0, greatest
 * matrix entry) its score is at most
 *     ub_top = s+ max(0, n - hi - 1) - 2 go - (2 (hi + 1) - (n - m) - 2) ge      if hi + 1 <= n
 *     ub_bot = s+ max(0, m + lo - 1) - 2 go - (2 (1 - lo) + (n - m) - 2) ge      if lo - 1 >= -m
 * and exact = 1 iff the banded score is STRICTLY above both, or neither applies (the band is the whole matrix).  Semiglobal rows get
 * 1 only when the band is the whole matrix.
 * CLH_ENDS_PREFIX and CLH_ENDS_EXTEND: without a hint the band is [-band, band] (the far end is free, n - m plays no part), with
 * diag[k] as above, clipped alike; row 0 is global's, the end cell is taken over the band's cells only.  create fails with
 * CLH_E_ARG for a band that misses (0, 0), lo > 0 or hi < 0, and for a prefix band with lo > n - m (no end cell on row m).  Every
 * cell (i, j) of an admitted band is reached from (0, 0): its diagonal d = j - i lies between 0 and itself inside the band, so row
 * 0 (d >= 0) or column 0 (d < 0) from (0, 0) to the diagonal, then the diagonal down to the cell, is a path in the band.  exact:
 * an alignment that leaves the band has a cell on diagonal hi + 1 or lo - 1 and need not come back.  Reaching hi + 1 from (0, 0)
 * takes at least hi + 1 D letters in at least one run, which leaves at most min(m, n - hi - 1) M columns; mirrored below:
 *     ub_top = s+ min(m, n - hi - 1) - go - hi ge        if hi + 1 <= n
 *     ub_bot = s+ min(n, m + lo - 1) - go - (-lo) ge     if lo - 1 >= -m
 * and exact = 1 iff the banded score is STRICTLY above every defined bound, or none is defined.  Then no cell outside the band
 * reaches the optimum, a band cell that reaches it in the full matrix does so by an alignment inside the band, so the best cells,
 * the tie among them and the walk are the same.  Host arithmetic in int64.  A pair with an empty side never reaches a kernel; fetch
 * states the boundary cell the band holds.  info: out[12] = {band positions a lane owns in class 0, 1, 2 (a pair is filed under the
 * first class whose 64 lanes hold its band), the greatest clipped width, shares of the batch, workspace bytes in use, those of the
 * largest pair, pairs the kernels take in class 0, 1, 2, pairs with an empty side, CIGAR ops fetch may return}.  Life cycle, error
 * codes, fetch's failures and `stream` as clh_ends_plan_*. */
typedef struct { int32_t mode; const int8_t* mat; int32_t n_mat; int32_t gap_open, gap_extend; int32_t want_cigar; int64_t workspace_bytes; int32_t band; int32_t reserved; } clh_band_opts;
typedef struct { int32_t score, ref_begin, ref_end, query_begin, query_end, cigar_len; int64_t cigar_off; int32_t band_lo, band_hi, exact, reserved; } clh_band_row;
typedef struct clh_band_plan clh_band_plan;
clh_band_plan* clh_band_plan_create(clh_ctx* ctx, int32_t n, const int8_t* q, const int64_t* q_off, const int8_t* r, const int64_t* r_off,
                                    const int32_t* diag, const clh_band_opts* opts);
void clh_band_plan_destroy(clh_band_plan* plan);
int clh_band_plan_run(clh_band_plan* plan, void* stream);
int clh_band_plan_fetch(clh_band_plan* plan, clh_band_row* rows, uint32_t* cigar, int64_t cigar_cap, int64_t* cigar_used);
int clh_band_plan_timing(clh_band_plan* plan, float* ms);     /* HIP events around the last run */
int clh_band_plan_info(clh_band_plan* plan, int64_t* out);
/* create + run + fetch */
int clh_band_batch(clh_ctx* ctx, int32_t n, const int8_t* q, const int64_t* q_off, const int8_t* r, const int64_t* r_off, const int32_t* diag,
                   const clh_band_opts* opts, clh_band_row* rows, uint32_t* cigar, int64_t cigar_cap, int64_t* cigar_used);
/* Two-piece gap costs over a band: clh_gap2 as for clh_ends_*_gap2, the band, its refusals, the modes and the rows as for clh_band_*.
 * The 2^29 bound takes the maximum over all four costs; stored decisions are one byte per cell of the band.  `exact` is the same
 * certificate with g(L) = min(gap_open + (L - 1) gap_extend, gap_open2 + (L - 1) gap_extend2) for the cost of a run of L letters:
 * global, ub_top = s+ max(0, n - hi - 1) - g(hi + 1) - g(hi + 1 - (n - m)) and ub_bot = s+ max(0, m + lo - 1) - g(1 - lo) - g(n - m -
 * lo + 1); free far end, ub_top = s+ min(m, n - hi - 1) - g(hi + 1) and ub_bot = s+ min(n, m + lo - 1) - g(1 - lo); the score must be
 * strictly above both.  The proof asks of g only that it does not decrease and that g(a) + g(b) >= g(a + b), which holds under the
 * admitted costs.  Every row with exact == 1 equals the row of clh_ends_*_gap2.  gap2 == NULL is clh_band_plan_create / clh_band_batch. */
clh_band_plan* clh_band_plan_create_gap2(clh_ctx* ctx, int32_t n, const int8_t* q, const int64_t* q_off, const int8_t* r, const int64_t* r_off,
                                         const int32_t* diag, const clh_band_opts* opts, const clh_gap2* gap2);
int clh_band_batch_gap2(clh_ctx* ctx, int32_t n, const int8_t* q, const int64_t* q_off, const int8_t* r, const int64_t* r_off, const int32_t* diag,
                        const clh_band_opts* opts, const clh_gap2* gap2, clh_band_row* rows, uint32_t* cigar, int64_t cigar_cap, int64_t* cigar_used);

/* ---- K1g and K1gb against windows of the resident genome ---------------------------------------------------------------------------
 * The plans above with reference k = the win_len[k] bases of the genome from win_off[k] (genome-wide offsets, as clh_ssw_plan_windows
 * takes them), read as win_flags[k] says: bit 0 reversed (letter t of the reference is base win_len - 1 - t of the window), bit 1
 * complemented; 3 is the minus strand, 1 the reversed flank of an extension to the left.  create gathers the windows on the device
 * into the plan's reference buffer (once; not per run) and returns a plan of the existing type: run, fetch, timing, info and destroy
 * are those above, and rows, ties and CIGARs are those of the strings form on the same letters.  The letters: A/a 0, C/c 1, G/g 2,
 * T/t 3, anything else 4, and complementing maps 0..3 to 3 - code WHATEVER THE CASE.  This differs on purpose from the windows of
 * clh_ssw_plan_windows, which leave a lower-case base of a minus-strand window uncomplemented as the reference's revcomp() does:
 * these modes have no call site in the reference to be bit-equal with, and a soft-masked minus-strand exon must align.
 * gap2, splice and strand may each be NULL (strand only comes with splice; gap2 together with splice is CLH_E_UNSUPPORTED, as
 * in the strings form).  The plan lives on the genome's context.  Refusals beyond those of the strings form: CLH_E_ARG for a null
 * genome, and, naming the first such pair, for win_len < 0, win_off < 0, win_off + win_len > clh_genome_length and flags above 3;
 * CLH_E_UNSUPPORTED for n_mat != 5 (substitution matrices over other alphabets take their references as strings). */
clh_ends_plan* clh_ends_plan_create_windows(clh_genome* genome, int32_t n, const int8_t* q, const int64_t* q_off, const int64_t* win_off,
                                            const int32_t* win_len, const uint8_t* win_flags, const clh_ends_opts* opts, const clh_gap2* gap2,
                                            const clh_splice* splice, const int8_t* strand);
clh_band_plan* clh_band_plan_create_windows(clh_genome* genome, int32_t n, const int8_t* q, const int64_t* q_off, const int64_t* win_off,
                                            const int32_t* win_len, const uint8_t* win_flags, const int32_t* diag, const clh_band_opts* opts,
                                            const clh_gap2* gap2);
/* HIP events around the gather that create ran, and the letters it moved (each read once and written once); CLH_E_ARG for a plan
 * whose references are strings or whose windows hold no letter. */
int clh_ends_plan_gather_timing(clh_ends_plan* plan, float* ms, int64_t* letters);
int clh_band_plan_gather_timing(clh_band_plan* plan, float* ms, int64_t* letters);

/* ---- K7: minimizer index of the resident genome, seeds and chains (csrc/seed.hip) ---------------------------
 * The producer of the loci the plans above take.  Nothing of it exists in the reference, whose mapper is an external package; the
 * definitions are this project's own, independent of the order positions are visited in, and stated in plain Python by
 * tests/seed_check.py, with which every array below is compared for equality.
 *
 * Minimizers, 4 <= k <= 28, 1 <= w <= 64.  A sequence is base codes (bits 0-2 of a resident byte, or a read code 0..4; 4 is no base).
 * Position p of a sequence of n letters (P = n - k + 1 positions) has a valid k-mer if its k codes are below 4 and its forward packing f
 * (2 bits per base, first base most significant) differs from the packing r of its reverse complement; strand = (f > r), key =
 * mix(min(f, r)), mix the 64-bit integer mix of seed_device.h (sd_mix) with every step masked to 2k bits.  With w' = min(w, P), p is a
 * minimizer iff it is valid and some window of w' consecutive positions inside [0, P) holds p and no valid key below key[p]: all ties
 * are selected.  A contig is a sequence of its own; no k-mer and no window spans two.
 *
 * clh_seed_index_create sketches the contigs [contig_off[c], contig_off[c] + contig_len[c]) of the genome (ascending, not overlapping,
 * inside it) on the device and sorts the entries by (key, genome-wide position).  Buffers are sized from the count pass.  CLH_E_ARG:
 * k, w or max_occ (>= 1) out of range, contigs out of order or outside the genome; CLH_E_CAPACITY with the bytes asked for: the
 * device refused an allocation.  The index lives on the genome's context and reads the genome in place: destroy it before the genome.
 *
 * clh_seed_index_info, out[12]: entries, distinct keys, keys with more than max_occ entries, device bytes held, k, w, max_occ, shares
 * of the last seeds / chains call, then the sketch's geometry: positions a wave decides per round, positions of a work item, work items
 * of a workgroup, and 0.  clh_seed_index_timing, ms[5] (HIP events): sketch and sort of the build, the last clh_seed_minimizers /
 * clh_seed_batch (sketch, look-up, sorts; no transfers to the host), the chain kernels of the last clh_seed_chain_batch, the link
 * kernels of the last clh_seed_link_batch / clh_seed_link_rows (below).
 * clh_seed_index_dump: entries [first, first + count) of the sorted arrays.
 *
 * clh_seed_minimizers: the same sketch on n sequences of codes 0..4; min_off[n + 1]; then clh_seed_minimizers_fetch(cap >= min_off[n])
 * gives position (inside the sequence), key and strand of each, in (sequence, position) order.
 *
 * clh_seed_batch: per read its minimizers, each looked up in the sorted keys; a key with more than max_occ entries gives no anchors and
 * counts in repetitive[read]; every other entry gives the anchor (read, minus, x, y): minus = strand of the read's k-mer XOR that of the
 * genome's, x the genome-wide start of the genome k-mer, y = q (the k-mer's start in the read) on the plus strand and L - k - q on the
 * minus strand (L the read's length): the start in the reverse-complemented read, so that on either strand a true alignment is a run
 * ascending in x and y.  anchor_off[n + 1]; clh_seed_batch_fetch(cap >= anchor_off[n]) gives the anchors in ascending (read, minus, x,
 * y) order.  A batch whose anchors need more than workspace_bytes (<= 0: 1 GiB; 64 bytes an anchor) is cut into shares of whole reads,
 * with the same arrays; one read above it is CLH_E_CAPACITY.  CLH_E_ARG, naming the first read: a code outside 0..4, a read of 2^24
 * letters or more.
 *
 * The two fetches read what their call parked on the index in host memory (16 B per minimizer or anchor), held until the next call of
 * the same kind or the index's destruction: a fetch follows its call directly, and one index serves one caller at a time -- two threads
 * sharing an index would overwrite each other's results; give each its own index or serialise call and fetch as a pair.
 *
 * clh_seed_chain_batch: the seeds step, then per segment (read, minus), anchors i = 0.. in the order above,
 *   f(i) = max(k, max_j f(j) + min(dx, dy, k) - beta(|dx - dy|)) over j in [i - lookback, i) on the same contig with dx = x_i - x_j > 0,
 *   dy = y_i - y_j > 0, dx, dy <= max_gap, |dx - dy| <= max_skew; beta(0) = 0, beta(d) = (k d + 99) / 100 + floor(log2 d) / 2;
 *   p(i) the nearest j attaining a value strictly above k, else -1.
 * Extraction, at most max_attempts times and until max_chains are out: e = the unused anchor of greatest f (ties: smallest index); stop
 * if f(e) < min_score; walk e, p(e), ... while unused, marking; score = f(e) - f(the used anchor the walk stopped on, if any); the chain
 * is emitted if score >= min_score and it holds >= min_anchors anchors.  A segment that has used max_attempts with such an e still
 * there is `truncated`.  seg[2 n][4]: chains, truncated, anchors, 0; rows[2 n][max_chains][10], the first `chains` of a segment written:
 * read, minus, contig, score, anchors, x_first, y_first, x_last + k, y_last + k, 0 (x relative to the contig; segment 2 r + minus).
 * 1 <= lookback <= 64, 1 <= max_chains <= 64, max_attempts >= 1, max_gap, max_skew >= 0, else CLH_E_ARG.  A row or header the kernel
 * left unwritten is CLH_E_HIP from this call, never returned.
 *
 * Links (csrc/seed_link.hip; the plain statement is tests/link_check.py): the chains of one segment, c = 0 .. n - 1 in the order the rows
 * hold them (n <= max_chains <= 64), each with g = contig, score, x0 = x_first, x1 = x_last + k, y0 = y_first, y1 = y_last + k, are
 * linked into paths.  The chains are ranked by the key (y0, y1, x0, c) ascending.  A link j -> i needs rank j < rank i and
 *   g_j == g_i, y0_i > y0_j, y1_i > y1_j; with q = y0_i - y1_j: q <= max_query_gap and -q <= max_overlap;
 *   with d = (x0_i - x1_j) - q exactly one kind: 1 colinear, |d| <= max_skew, cost beta(|d|) as above; 2 intron, max_skew < d <=
 *   max_intron, cost intron_cost; 3 back-splice, d < -max_skew and 0 < x1_j - x0_i <= max_circle, cost backsplice_cost; anything else
 *   is no link.
 * v(j, i) = F_j - cost - max(0, -q); F_i = score_i + max(0, max_j v(j, i)); pred_i the j of the maximum and kind_i its kind, -1 and 0
 * where no link has v > 0; among equal maxima the j of greatest rank.  Paths, until every chain is in one: e = the chain in no path of
 * greatest F (ties: smallest rank); walk e, pred(e), ... up to a chain already in a path or to none; the chains walked are path p = 0,
 * 1, ... in the order of extraction, pos counting from the path's first chain (the last one walked); the path's score is F_e - F of the
 * chain the walk stopped on (0 where on none).  No threshold is applied.
 * link_seg[nseg][4]: chains, paths, 0, 0; link_rows[nseg][max_chains][8], the first `chains` of a segment written: rank, F, pred, kind,
 * path, pos, the path's score where pos == 0 else 0, 0.
 * clh_link_opts: every field >= 0, max_skew <= max_intron, the two costs below 2^40, else CLH_E_ARG.
 * clh_seed_link_batch: clh_seed_chain_batch, then the links of every segment (2 r + minus) on the device rows, in the same shares and
 * with no trip to the host between the two; seg and rows are those of clh_seed_chain_batch.  clh_seed_index_timing gives ms[5]: the
 * four above and the link kernels of the last clh_seed_link_batch / clh_seed_link_rows (the kernels alone: the marker fill of their
 * rows lies outside the interval).
 * clh_seed_link_rows: the links of nseg segments of chain rows that the caller gives (another mapper's hits): seg[nseg][4] with the
 * count in its first word, rows[nseg][max_chains][10] in the layout above, of which contig, score, x_first, y_first, x_end and y_end
 * are read.  The index gives its context and k.  CLH_E_ARG, naming the segment: a count outside 0..max_chains, a coordinate outside
 * [0, 2^40), a score outside (-2^40, 2^40).  Every buffer is sized from the arguments.  As above, a header or row the kernel left
 * unwritten, or a walk that would have left the segment, is CLH_E_HIP, never returned. */
typedef struct clh_seed_index clh_seed_index;
typedef struct {
    int32_t lookback, max_chains, max_attempts, min_score, min_anchors, reserved;
    int64_t max_gap, max_skew, workspace_bytes;
} clh_chain_opts;
clh_seed_index* clh_seed_index_create(clh_genome* genome, int32_t k, int32_t w, int32_t n_contigs, const int64_t* contig_off, const int64_t* contig_len,
                                      int32_t max_occ);
void clh_seed_index_destroy(clh_seed_index* index);
int clh_seed_index_info(clh_seed_index* index, int64_t* out);
int clh_seed_index_timing(clh_seed_index* index, float* ms);
int clh_seed_index_dump(clh_seed_index* index, int64_t first, int64_t count, uint64_t* keys, int64_t* pos, uint8_t* strand);
int clh_seed_minimizers(clh_seed_index* index, int32_t n, const int8_t* seqs, const int64_t* seq_off, int64_t* min_off);
int clh_seed_minimizers_fetch(clh_seed_index* index, int64_t cap, int64_t* pos, uint64_t* keys, uint8_t* strand);
int clh_seed_batch(clh_seed_index* index, int32_t n, const int8_t* reads, const int64_t* read_off, int64_t workspace_bytes, int64_t* anchor_off,
                   int32_t* repetitive);
int clh_seed_batch_fetch(clh_seed_index* index, int64_t cap, int32_t* read, uint8_t* minus, int64_t* x, int32_t* y);
int clh_seed_chain_batch(clh_seed_index* index, int32_t n, const int8_t* reads, const int64_t* read_off, const clh_chain_opts* opts, int64_t* seg,
                         int64_t* rows);
typedef struct {
    int64_t max_query_gap, max_overlap, max_skew, max_intron, max_circle, intron_cost, backsplice_cost;
} clh_link_opts;
int clh_seed_link_batch(clh_seed_index* index, int32_t n, const int8_t* reads, const int64_t* read_off, const clh_chain_opts* chain_opts,
                        const clh_link_opts* link_opts, int64_t* seg, int64_t* rows, int64_t* link_seg, int64_t* link_rows);
int clh_seed_link_rows(clh_seed_index* index, int32_t nseg, int32_t max_chains, const int64_t* seg, const int64_t* rows, const clh_link_opts* link_opts,
                       int64_t* link_seg, int64_t* link_rows);

/* ---- K7j: a back-splice junction refined to the base (csrc/seed_junction.hip) -------------------------------
 * The plain statement is tests/junction_check.py.  The definition is the project's own; parity with find_bsj.py's rotate-and-map loop,
 * clip alignment and sliding signal search is neither sought nor claimed.
 *
 * A task (8 int64: read, minus, contig, xd, yd, xa, ya, strand) is one back-splice, given by two anchor points on one contig and one
 * strand of one read.  S is the read as the strand reads it: for minus != 0 the reverse complement of the read as given (codes below 4
 * complemented, 4 stays 4), K7's y frame.  The donor anchor (xd, yd) is a point known to be aligned on the side the read leaves, the
 * acceptor anchor (xa, ya) one on the side it re-enters; both x are relative to the contig.  From a link j -> i of kind 3 the anchors
 * are xd = x1_j - k, yd = y1_j - k (the start of the source chain's last k-mer) and xa = x0_i + k, ya = y0_i + k (the end of the target
 * chain's first k-mer).  With m = ya - yd:
 *   Q = S[yd : ya);  D = contig[xd : min(xd + m + slack, contig_len)), nD letters forward from the donor anchor;
 *   A = contig[max(0, xa - m - slack) : xa), nA letters up to the acceptor anchor.
 * Genome letters are bits 0-2 of the resident byte, clamped to 4, the case dropped; no letter of a neighbouring contig is read.
 *   HL[t][u], 0 <= t <= m, 0 <= u <= nD: the global affine score of Q[0:t) against D[0:u);
 *   HR[t][v], 0 <= v <= nA: the global affine score of Q[t:m) against the last v letters of A;
 * equal codes below 4 score +match, everything else (code 4 on either side included) -mismatch; a gap of g letters costs gap_open +
 * (g - 1) gap_extend, gap_open >= gap_extend: K1g's one-piece recurrences with global boundaries.
 * The skipped run starts at a = xd + u and ends at b = xa - v - 1, and clh_splice prices it as in clh_ends_plan_create_spliced: strand +:
 * start = donor[r[a], r[a + 1]], end = acceptor[r[b - 1], r[b]]; strand -: start = acceptor[c(r[a + 1]), c(r[a])], end = donor[c(r[b]),
 * c(r[b - 1])]; a dinucleotide that holds a code >= 4 or leaves the contig costs `other`.
 *   J(s, t, u, v) = HL[t][u] + HR[t][v] - start_s(xd + u) - end_s(xa - v - 1) - intron_open
 * and the answer is its maximum over the task's strands (strand +1, -1, or 0 for both); ties go to strand +, then the smallest t, then
 * the smallest u, then the smallest v.
 * out[n_tasks][12]: status, score, strand (0 +, 1 -), t, u, v, donor_end = xd + u (the circle's exclusive end), acceptor_start = xa - v
 * (its 0-based start), HL[t][u], HR[t][v], the start cost, the end cost.  status 0: refined; 1: m > max_span, not attempted; 2: m < 1 or
 * xa >= xd, the anchors cross (where both hold, 1); for 1 and 2 the other eleven words are 0.  With xa < xd, acceptor_start < donor_end.
 * Limits: 1 <= max_span <= 512, 0 <= slack <= 64, every cost >= 0, and (2 max_span + slack) max(match, mismatch, gap_open, gap_extend) +
 * intron_open + dmax + amax < 2^20 (dmax, amax the greatest donor and acceptor cost, `other` included): under it a side score less a site
 * cost lies inside (-2^20, 2^20), and such a value and a column index share one 32-bit key in the kernel.  Outside these CLH_E_ARG;
 * gap_open < gap_extend is CLH_E_UNSUPPORTED.  CLH_E_ARG, naming the first read or task: a read code outside 0..4; a read index or
 * contig out of range, yd or ya outside [0, L], xd or xa outside [0, contig_len], a strand outside {-1, 0, 1}.  A row the kernel left
 * unwritten is CLH_E_HIP, never returned.  n_tasks == 0 is success.  kernel_ms (may be NULL): HIP events around the kernels alone.
 * clh_seed_junction_info, out[8]: the four class bounds on m (a class of bound 64 c gives a lane c rows), the greatest max_span, the
 * greatest slack, the waves (tasks) of a workgroup, the number of classes. */
typedef struct { int32_t match, mismatch, gap_open, gap_extend, slack, max_span; } clh_junction_opts;
int clh_seed_junction_batch(clh_seed_index* index, int32_t n_reads, const int8_t* reads, const int64_t* read_off, int64_t n_tasks,
                            const int64_t* task, const clh_junction_opts* opts, const clh_splice* splice, int64_t* out, float* kernel_ms);
int clh_seed_junction_info(int64_t* out);

/* ---- K7c: the circles of a read batch in one device pass, with read counts (csrc/seed_circle.hip) ---------
 * The plain statement is tests/circle_check.py.  The reads are uploaded once; sketch, look-up, chains, links, the best path of every read,
 * its K7j tasks, K7j, the flanking dinucleotides and the table of the distinct circles all run on the device, in the shares of
 * clh_seed_link_batch, and what comes back is one row of 16 words per read and one row per distinct circle.  The definitions restate what
 * clh_seed_link_batch, the host steps of ciri_long_amd.seed.call_circles and clh_seed_junction_batch compute between them, k the index's
 * k-mer length.  For read r of L letters, its segments 2 r (plus) and 2 r + 1 (minus) linked as clh_seed_link_batch links them:
 *   Best path.  The candidates are the paths of both segments whose score (link_rows[..][6] at pos == 0) is at least min_path_score (which
 *     may be negative); the best is the least under (-score, minus, x_first of the path's pos-0 chain, path index).  None: status 1.
 *   Tasks.  Every chain i of that path with kind == 3 and j = pred_i, in ascending pos, gives the task
 *     (r, minus, contig, x1_j - k, y1_j - k, x0_i + k, y0_i + k, 0).  None: status 2.
 *   Junctions.  Each task is answered by K7j exactly as clh_seed_junction_batch answers it (above).
 *   Winner.  Among the tasks of K7j status 0 the one of greatest J, among equals the first in path order.  None: status 3.
 *   Flanks.  after = contig[donor_end : donor_end + 2), before = contig[acceptor_start - 2 : acceptor_start), letters as K7j reads them.
 *     Strand +: donor = after, acceptor = before; strand -: donor = revcomp(before), acceptor = revcomp(after), code 4 stays 4.  A
 *     dinucleotide is coded 5 c0 + c1, and -1 where fewer than two of its letters lie inside the contig.
 *   read_pos.  With y = yd + t: L - y on the minus strand, y otherwise: the split in the read as given.
 * circle[n][16]: status 0-3, contig, start (acceptor_start), end (donor_end, exclusive), strand (0 +, 1 -), donor code, acceptor code, J,
 * read_pos, the path's minus, the path's score, chains in the path, its back-splice links, how many of those K7j refined, the winner's
 * ordinal among them, 0.  At status 1 words 1-14 are 0; at status 2 and 3 words 9-13 are filled and the rest are 0.
 * The table groups the status-0 rows by (contig, start, end, strand) exactly: table[n_circles][10] = contig, start, end, strand, donor,
 * acceptor, reads (the count), the greatest J, the lowest read index, 0, ascending in (contig, start, end, strand);
 * circle_of_read[n] is a read's row in the table, or -1.  The grouping runs over the rows of the whole batch after the last share and does
 * not depend on how the batch was cut.  clh_seed_circle_table_fetch(cap >= n_circles) gives the table of the last call (the convention
 * of clh_seed_batch_fetch); a cap too small is CLH_E_CAPACITY.
 * The call refuses what clh_seed_link_batch and clh_seed_junction_batch refuse, with their codes; an index of 2^23 contigs or more is
 * CLH_E_CAPACITY; n == 0 is success with n_circles = 0.  Capacity goes through chain_opts->workspace_bytes as in clh_seed_link_batch;
 * a read owns max(max_chains - 1, 1) task slots (160 bytes each) of its share, and an allocation the device refuses is CLH_E_CAPACITY
 * with its byte count.  Every index a kernel takes from a row is checked before it is followed; a read whose rows fail, and any row left
 * unwritten, is CLH_E_HIP, never returned.  kernel_ms (float[3], may be NULL): HIP events around the select / task-build kernels, the
 * junction kernels, and the finalise and table kernels alone, summed over the shares.  Between the first two, kJxClasses task counters
 * come back to the host per share, by which the junction launches are sized; the paths and the tasks do not come back.
 * clh_seed_index_timing keeps its five slots: seeds, chain and link are those of this call's shares. */
int clh_seed_circle_batch(clh_seed_index* index, int32_t n, const int8_t* reads, const int64_t* read_off, const clh_chain_opts* chain_opts,
                          const clh_link_opts* link_opts, const clh_junction_opts* junction_opts, const clh_splice* splice, int64_t min_path_score,
                          int64_t* circle, int64_t* circle_of_read, int64_t* n_circles, float* kernel_ms);
int clh_seed_circle_table_fetch(clh_seed_index* index, int64_t cap, int64_t* table);


/* ASCII -> codes exactly as ssw_wrap.py:234-252 (A/a C/c G/g T/t N/n, anything else 4), on the host. */
void clh_encode_dna(const char* seq, int64_t len, int8_t* out);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
