/*
 * ccs_oracle.c -- CPU statement of the cyclic-consensus step (find_consensus) as THIS repository defines it.
 *
 * TEST INFRASTRUCTURE ONLY (same rules as ssw_oracle.c).
 *
 * PARITY UNPINNED.  CIRI-long delegates this step to the external packages pyccs (find_consensus) and spoa (poa)
 * (CIRI_long/find_ccs.py:8,14; setup.py:57).  Neither their sources nor their wheels exist in /root/reference or in
 * this environment, and the reference's only test of them asserts one length (tests/test_poa.py:32).  There is no file
 * to restate and no output to compare with.  What follows is therefore a specification written for this project from
 * the published description of the method (k-mer self-matches give the repeat period; the read is cut into copies;
 * the copies are combined by partial-order alignment), fixed in every detail so that the HIP kernels (K2 ccs_scan, K3
 * poa_consensus) can be checked bit for bit against it.  It reproduces the CONTRACT the reference consumes:
 * `(segments, ccs)` with segments "s0-e0;s1-e1;..." ascending on the raw read, or (None, None)
 * (find_ccs.py:14-16,94; find_bsj.py:254-255).
 *
 * Specification "clh-ccs v2"
 * --------------------------
 * codes: A0 C1 G2 T3, anything else 4.  A k-mer is valid if it holds no code 4.
 * 1. period.  k = 8 (4^8 codes: a 1 kb read has ~0.01 chance matches per offset, while 13 % sequencing error leaves
 *    ~10 % of true 8-mer pairs intact).  cnt[d] = #{ i : kmer(i), kmer(i+d) valid and equal }, d in [30, L/2];
 *    s[d] = sum of cnt over [d-3, d+3] (clipped to the range); p0 = smallest d with maximal s[d].
 *    s[p0] < 12 -> there is no repeat.  Harmonics: for q = 2..8 while (p0+q/2)/q >= 30, let e be the offset with the
 *    largest s in [(p0+q/2)/q - 3, +3] (smallest on ties); if 2*s[e] >= s[p0] the period is e; the largest such q wins
 *    (noise can lift 2p or 3p slightly above p).
 * 2. copies.  Every cut is the position homologous to the previous cut one copy later, read off the exact k-mer recurrence
 *    ("anchor") that sits nearest to the previous cut -- so all copies start at the phase of the read's first base.
 *    tol = max(4, p0/8), W = min(p0, 96).  b = 0, prev = p0.  Repeat: candidates delta in [p0-tol, p0+tol] with
 *    b+delta <= L; none -> stop.  An anchor is a pair (i, delta): i in [max(0, b-W), b+W), delta a candidate, kmer(i) and
 *    kmer(i+delta) valid and equal (same k as step 1).
 *      a. vote.  score(delta) = number of anchors with that delta; v = the delta with the best score; ties: smallest
 *         |delta-prev|, then smallest delta.  (Without any anchor that is the candidate closest to prev, and the cut is b+v.)
 *      b. anchor.  Among the anchors with |delta-v| <= 8 (a chance recurrence of an 8-mer elsewhere in the tolerance
 *         window is not followed) take the one whose k-mer centre lies nearest to b: smallest |i+4-b|, then the larger i,
 *         then smallest |delta-prev|, then smallest delta.  Cut at b+delta, prev = delta.
 *    At most 64 cuts.  Fewer than 2 full copies -> no repeat.  A tail of >= 20 bases after the last cut is kept as a
 *    partial copy, unless the 64-cut cap ended the search (the rest of the read is then an unscanned stretch of copies and
 *    is left out).
 *    v1 (rounds 1-5) cut at b+v, the vote over [b, b+W) alone.  The most frequent offset of a window is not the offset AT b:
 *    whenever the next copy has lost bases inside the window the cut slid into the previous copy (2 to 9 bases on the one
 *    segmentation of pyccs the reference holds, the six strings of tests/test_poa.py:8-15, whose concatenation v2 cuts at
 *    their own lengths 145;289;433;577;713;751 -- tests/test_ccs_oracle.py asserts it).  On synthetic reads, where the
 *    generator knows the truth, the mean distance of a cut from the true copy start falls from 2.75 to 1.71 bases
 *    (tools/dev/ccs_cut_eval.py).  Still PARITY UNPINNED: this is the rule that reproduces the only evidence there is.
 *    (Until round 4 a copy longer than 2800 bases gave no consensus -- a limit of the alignment kernel's 16-bit cells written into
 *    the specification.  pyccs has no reason to refuse such a read; the kernel now has a wide form of its pass and the limit is gone.)
 * 3. consensus.  Partial-order alignment of the copies in read order (poa_oracle.c), heaviest bundle, restricted to the
 *    nodes crossed by at least (copies + 1) / 2 of the copies (the partial last copy counts as a copy).
 *
 * Step 3 is spoa.poa(copies, 0, ., 10, -4, -8, -2, -24, -1) -- local alignment, two-piece gap cost, the call of the
 * reference's tests/test_poa.py:30, whose assertion (:32) equates the length of that consensus with the length of
 * find_consensus' -- as stated in poa_oracle.c ("clh-poa v3": a restatement of the published spoa algorithm).
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define CCS_K 8
#define CCS_DMIN 30
#define CCS_MIN_SUPPORT 12
#define CCS_SMOOTH 3
#define CCS_MAX_CUTS 64
#define CCS_MIN_TAIL 20
#define CCS_GUARD 8

static inline int imax(int a, int b) { return a > b ? a : b; }
static inline int imin(int a, int b) { return a < b ? a : b; }

/* k-mer codes; -1 = invalid */
static void kmer_codes(const int8_t *seq, int L, int k, int32_t *h)
{
    for (int i = 0; i < L; ++i) h[i] = -1;
    for (int i = 0; i + k <= L; ++i) {
        int32_t c = 0, ok = 1;
        for (int t = 0; t < k; ++t) {
            int b = seq[i + t];
            if (b < 0 || b > 3) { ok = 0; break; }
            c = (c << 2) | b;
        }
        h[i] = ok ? c : -1;
    }
}

/* What a run of the step decided and how close each decision was (clo_ccs_trace; tests/ccs_edges.py builds its inputs on it).
   period[]: bestd, best, offsets tied at best, harmonics evaluated, cuts made, p0, 0, 0, then per evaluated q: q, e, s[e], 2*s[e] - best.
   cut[n][]: b, lo, hi | the vote v, its score, deltas with that score, of those with the same |delta - prev| | did the anchor stage
   run | the chosen i, delta and its dist | anchors at the minimal dist, of those with the same i, of those with the same |delta - prev|. */
#define CLO_CCS_TRACE_PERIOD 40
#define CLO_CCS_TRACE_CUT 16
typedef struct { int32_t *period, *cut; } ccs_trace_t;

/* step 1+2.  cuts[0..ncuts) are the boundaries after 0 (b1, b2, ...); returns period or 0.  tr: optional record of the run */
static int ccs_segments(const int8_t *seq, int32_t L, int32_t *cuts, int32_t *ncuts, int32_t *k_used, int32_t *support, const ccs_trace_t *tr)
{
    *ncuts = 0; *k_used = 0; *support = 0;
    if (L < 2 * CCS_DMIN) return 0;
    int32_t *h = (int32_t *)malloc(sizeof(int32_t) * (size_t)L);
    int32_t *cnt = (int32_t *)calloc((size_t)L / 2 + 2, sizeof(int32_t));
    int p0 = 0, kk = 0;
    const int ks[1] = {8};
    for (int a = 0; a < 1 && !p0; ++a) {
        int k = ks[a];
        kmer_codes(seq, L, k, h);
        int dmax = L / 2;
        for (int d = CCS_DMIN; d <= dmax; ++d) {
            int c = 0;
            for (int i = 0; i + d < L; ++i) c += (h[i] >= 0 && h[i] == h[i + d]);
            cnt[d] = c;
        }
        int32_t *sm = (int32_t *)calloc((size_t)dmax + 2, sizeof(int32_t));
        int best = -1, bestd = 0;
        for (int d = CCS_DMIN; d <= dmax; ++d) {
            int s = 0;
            for (int e = imax(d - CCS_SMOOTH, CCS_DMIN); e <= imin(d + CCS_SMOOTH, dmax); ++e) s += cnt[e];
            sm[d] = s;
            if (s > best) { best = s; bestd = d; }
        }
        if (tr) {
            int tied = 0;
            for (int d = CCS_DMIN; d <= dmax; ++d) tied += sm[d] == best;
            tr->period[0] = bestd; tr->period[1] = best; tr->period[2] = tied; tr->period[3] = 0;
        }
        if (best >= CCS_MIN_SUPPORT) {
            p0 = bestd; kk = k; *support = best;
            for (int q = 2; q <= 8; ++q) {                     /* harmonics: prefer the fundamental */
                const int c = (bestd + q / 2) / q;
                if (c < CCS_DMIN) break;
                int eb = -1, es = -1;
                for (int e = imax(c - 3, CCS_DMIN); e <= imin(c + 3, dmax); ++e) if (sm[e] > es) { es = sm[e]; eb = e; }
                if (eb >= 0 && 2 * es >= best) p0 = eb;
                if (tr) { int32_t *r = tr->period + 8 + 4 * tr->period[3]++; r[0] = q; r[1] = eb; r[2] = es; r[3] = 2 * es - best; }
            }
        }
        free(sm);
    }
    if (!p0) { free(h); free(cnt); return 0; }
    *k_used = kk;
    int tol = imax(4, p0 / 8), W = imin(p0, 96);
    int b = 0, prev = p0, n = 0;
    int32_t *hist = (int32_t *)malloc(sizeof(int32_t) * (size_t)(2 * tol + 1));
    while (n < CCS_MAX_CUTS) {
        const int lo = p0 - tol, hi = imin(p0 + tol, L - b);          /* lo >= 26: p0 >= 30 */
        if (hi < lo) break;
        const int i0 = imax(0, b - W), i1 = imin(L, b + W);
        /* a. the vote */
        for (int t = 0; t <= hi - lo; ++t) hist[t] = 0;
        for (int i = i0; i < i1; ++i) {
            if (h[i] < 0) continue;
            for (int delta = lo; delta <= hi && i + delta < L; ++delta) hist[delta - lo] += (h[i + delta] == h[i]);
        }
        int v = lo, vs = -1;
        for (int delta = lo; delta <= hi; ++delta) {
            const int sc = hist[delta - lo];
            if (sc > vs || (sc == vs && abs(delta - prev) < abs(v - prev))) { vs = sc; v = delta; }   /* equal distance keeps the smaller delta */
        }
        int cut = v;
        int32_t *r = tr ? tr->cut + CLO_CCS_TRACE_CUT * n : NULL;
        if (r) {
            memset(r, 0, sizeof(int32_t) * CLO_CCS_TRACE_CUT);
            r[0] = b; r[1] = lo; r[2] = hi; r[3] = v; r[4] = vs; r[7] = vs > 0; r[8] = -1; r[9] = v; r[10] = -1;
            for (int delta = lo; delta <= hi; ++delta)
                if (hist[delta - lo] == vs) { ++r[5]; r[6] += abs(delta - prev) == abs(v - prev); }
        }
        if (vs > 0) {
            /* b. the anchor nearest to b among those the vote does not rule out */
            int bd = 1 << 30, bi = -1, ba = 0, bdel = 0;
            for (int i = i0; i < i1; ++i) {
                if (h[i] < 0) continue;
                const int dist = abs(i + CCS_K / 2 - b);
                for (int delta = imax(lo, v - CCS_GUARD); delta <= imin(hi, v + CCS_GUARD) && i + delta < L; ++delta) {
                    if (h[i + delta] != h[i]) continue;
                    const int a = abs(delta - prev);
                    if (dist < bd || (dist == bd && (i > bi || (i == bi && a < ba)))) { bd = dist; bi = i; ba = a; bdel = delta; }   /* ascending delta: equal |delta-prev| keeps the smaller */
                }
            }
            cut = bdel;
            if (r) {
                r[8] = bi; r[9] = bdel; r[10] = bd;
                for (int i = i0; i < i1; ++i) {
                    if (h[i] < 0 || abs(i + CCS_K / 2 - b) != bd) continue;
                    for (int delta = imax(lo, v - CCS_GUARD); delta <= imin(hi, v + CCS_GUARD) && i + delta < L; ++delta) {
                        if (h[i + delta] != h[i]) continue;
                        ++r[11];
                        if (i == bi) { ++r[12]; r[13] += abs(delta - prev) == ba; }
                    }
                }
            }
        }
        b += cut;
        prev = cut;
        cuts[n++] = b;
    }
    free(hist);
    free(h); free(cnt);
    *ncuts = n;
    if (tr) { tr->period[4] = n; tr->period[5] = p0; }
    if (n < 2) { *ncuts = 0; return 0; }
    return p0;
}

int clo_ccs_segments(const int8_t *seq, int32_t L, int32_t *cuts, int32_t *ncuts, int32_t *k_used, int32_t *support)
{
    return ccs_segments(seq, L, cuts, ncuts, k_used, support, NULL);
}

/* the same run with its record: period[CLO_CCS_TRACE_PERIOD], cut[CCS_MAX_CUTS][CLO_CCS_TRACE_CUT] (rows of the cuts made, also where
   fewer than two of them leave the read without a repeat) */
int clo_ccs_trace(const int8_t *seq, int32_t L, int32_t *cuts, int32_t *ncuts, int32_t *k_used, int32_t *support, int32_t *period, int32_t *cut)
{
    const ccs_trace_t tr = {period, cut};
    memset(period, 0, sizeof(int32_t) * CLO_CCS_TRACE_PERIOD);
    return ccs_segments(seq, L, cuts, ncuts, k_used, support, &tr);
}

/* step 3 lives in poa_oracle.c */
int clo_poa(int32_t nseq, const int8_t *seqs, const int32_t *off, const int32_t *params, int8_t *cons, int32_t cap,
            int8_t *msa, int64_t msa_cap, int32_t *ncols, int32_t *scores);


/* find_consensus: segs[2*i], segs[2*i+1] = start, end of copy i.  returns consensus length, 0 = no repeat, -1 = error */
int clo_find_consensus(const int8_t *seq, int32_t L, int32_t *segs, int32_t *nseg, int8_t *ccs, int32_t cap, int32_t *period)
{
    int32_t cuts[CCS_MAX_CUTS], nc = 0, k = 0, sup = 0;
    *nseg = 0; *period = 0;
    const int p0 = clo_ccs_segments(seq, L, cuts, &nc, &k, &sup);
    if (!p0) return 0;
    *period = p0;
    int n = 0, b = 0;
    for (int i = 0; i < nc; ++i) { segs[2 * n] = b; segs[2 * n + 1] = cuts[i]; b = cuts[i]; ++n; }
    /* the rest of the read is a (partial) last copy -- unless the boundary search stopped at its cap, in which case the rest
       is an unscanned stretch of many copies and is left out */
    if (L - b >= CCS_MIN_TAIL && nc < CCS_MAX_CUTS) { segs[2 * n] = b; segs[2 * n + 1] = L; ++n; }
    *nseg = n;
    int32_t *off = (int32_t *)malloc(sizeof(int32_t) * (size_t)(n + 1));
    int8_t *buf = (int8_t *)malloc((size_t)L + 1);
    off[0] = 0;
    for (int i = 0; i < n; ++i) {
        memcpy(buf + off[i], seq + segs[2 * i], (size_t)(segs[2 * i + 1] - segs[2 * i]));
        off[i + 1] = off[i] + segs[2 * i + 1] - segs[2 * i];
    }
    /* local alignment, the scores of tests/test_poa.py:30; nodes crossed by fewer than half of the copies are left out of
       the consensus (the unaligned overhang of a copy cut a few bases early or late would otherwise lead or trail it) */
    const int32_t par[8] = {0, 10, -4, -8, -2, -24, -1, (n + 1) / 2};
    const int len = clo_poa(n, buf, off, par, ccs, cap, NULL, 0, NULL, NULL);
    free(off); free(buf);
    if (len < 0) { *nseg = 0; return -1; }
    return len;
}
