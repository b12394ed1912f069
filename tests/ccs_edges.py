"""Deterministic inputs for K2 (the repeat scan of csrc/ccs_poa.hip: ccs_scan_kernel, ccs_scan_kernel_x4, ccs_scan_long_kernel) through
Context.ccs_batch, each built for one named edge of the kernel (not a test module): the launch classes and their bucket counts, the
support, length and tail thresholds, periods at CCS_DMIN and at L/2, plateaus of the smoothed count that lie across lanes, strides and
waves, harmonics at a margin of 0 and -1, the cap of 64 cuts, ties of the vote and of the anchor's four keys, N and codes outside
0..4, and reads whose positions share one, two or three chains.

The limits come from constants parsed out of the sources (tools/ccs_scan_model.constants()); the templates' own lengths (40, 60, 80,
100 bases) are chosen so that tol, W and the guard take the values each case names, which the host proofs assert.  Expected values are
oracle/ccs_oracle.c; tests/test_ccs_edges_host.py proves from the oracle's own trace (oracle_lib.oracle_ccs_trace) that every case
reaches what its `what` names, tests/test_gpu_ccs_edges.py holds the kernels to the cases.

A case is Case(read, what): `read` an int8 array of codes (A0 C1 G2 T3, N 4), `what` a dict that names the edge.  Low-complexity reads
stay at or below 1100 bases: K2 visits every pair of equal 8-mers, L^2/2 chain steps in one workgroup for a homopolymer."""
import collections
import os
import random
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
import ccs_scan_model as M  # noqa: E402

Case = collections.namedtuple('Case', 'read what')
constants = M.constants


def _rng(*key):
    return random.Random('ccs edges ' + ' '.join(str(k) for k in key))


def dna(rng, n):
    return np.array([rng.randrange(4) for _ in range(n)], dtype=np.int8)


def tandem(unit, L):
    """exact copies of `unit`, cut to L bases"""
    return np.tile(unit, L // len(unit) + 1)[:L].copy()


def unit_of(p, *key):
    """a random template of p bases in which no 8-mer occurs twice"""
    for attempt in range(100):
        u = dna(_rng('unit', p, attempt, *key), p)
        uu = np.concatenate([u, u[:7]])
        kmers = {bytes(uu[i:i + 8]) for i in range(p)}
        if len(kmers) == p:
            return u
    raise ValueError('ccs_edges: no template of %d bases without a repeated 8-mer' % p)


def substitute(read, positions):
    read = read.copy()
    for p in positions:
        read[p] = (read[p] + 1) & 3
    return read


# ----------------------------------------------------------------------------------------------------------------------------
# 1. launch classes: lengths on both sides of every class, bucket and kernel boundary
# ----------------------------------------------------------------------------------------------------------------------------
def class_lengths(K):
    wide, ldsmax = K['K2_WIDE_FROM'], K['kK2LdsMax']
    (b1, _), (b2, _) = K['BUCKET_STEPS']
    return [wide - 64, wide - 63, wide - 1, wide, wide + 1, b1, b1 + 1, b2, b2 + 1, ldsmax, ldsmax + 1]


SECOND_LONG = 500           # the second read of the long kernel is this much longer than the first


def classes(K):
    """a repeat of period 203 (odd, so copies end off every power of two) cut to each class length; 'long' marks reads of the HBM kernel"""
    u = unit_of(203, 'classes')
    out = [Case(tandem(u, L), {'length': L, 'long': L > K['kK2LdsMax']}) for L in class_lengths(K)]
    L2 = K['kK2LdsMax'] + SECOND_LONG
    out.append(Case(tandem(unit_of(211, 'classes second'), L2), {'length': L2, 'long': True, 'second_long': True}))
    return out


def mixed_order(n):
    order = list(range(n))
    _rng('mixed batch').shuffle(order)
    return order


# ----------------------------------------------------------------------------------------------------------------------------
# 2. thresholds: support 11 | 12, L 59 | 60, L = 2p - 1 | 2p, one copy and a part
# ----------------------------------------------------------------------------------------------------------------------------
SUPPORT_SEED = 5


def planted(n, at=100, gap=50, L=200, seed=SUPPORT_SEED):
    """a random read of L bases whose n bases at `at` occur again `gap` later: n - 7 pairs of equal 8-mers at one offset"""
    r = dna(_rng('planted', seed), L)
    r[at + gap:at + gap + n] = r[at:at + n]
    return r


def thresholds(K):
    sup, dmin, k = K['CCS_MIN_SUPPORT'], K['CCS_DMIN'], K['CCS_K']
    out = [Case(planted(sup + k - 1), {'support': sup, 'period': 47}),
           Case(planted(sup + k - 2), {'support': sup - 1, 'period': 0})]
    u = unit_of(dmin, 'L60')
    out += [Case(tandem(u, 2 * dmin - 1), {'length': 2 * dmin - 1, 'period': 0}),
            Case(tandem(u, 2 * dmin), {'length': 2 * dmin, 'period': dmin, 'ncuts': 2})]
    u = unit_of(100, 'two copies')
    out += [Case(tandem(u, 200), {'two_copies': 200, 'period': 97, 'ncuts': 2}),
            Case(tandem(u, 199), {'two_copies': 199, 'period': 0}),
            # one full copy and too little of the second for a second cut: the offset of the repeat lies above L/2, so nothing is counted.
            # (The `n < 2` exit behind the cuts cannot be taken: bestd <= L/2 and p0 <= bestd leave L - cut1 >= 2 bestd - p0 - tol >= dlo.)
            Case(tandem(u, 187), {'few_cuts': True, 'period': 0})]
    return out


# ----------------------------------------------------------------------------------------------------------------------------
# 3. periods at the limits: below and at CCS_DMIN (smoothing clipped below), at L/2 (clipped above), the last k-mer of the read
# ----------------------------------------------------------------------------------------------------------------------------
def period_limits(K):
    dmin, k, sup = K['CCS_DMIN'], K['CCS_K'], K['CCS_MIN_SUPPORT']
    out = [Case(tandem(unit_of(dmin - 1, 'below'), 10 * (dmin - 1) + 10), {'unit': dmin - 1, 'multiple': True})]
    for p in (dmin, dmin + 1, dmin + 3, dmin + 4):
        out.append(Case(tandem(unit_of(p, 'dmin'), 9 * p + 5), {'unit': p, 'clipped_at_dmin': True}))
    u = unit_of(100, 'dmax')
    for extra in range(7):
        out.append(Case(tandem(u, 200 + extra), {'unit': 100, 'extra': extra, 'clipped_at_dmax': extra < 6}))
    # the read ends with the second occurrence: the pair whose second k-mer starts at L - 8 is one of exactly CCS_MIN_SUPPORT
    n = sup + k - 1
    out.append(Case(planted(n, at=200 - n - 50), {'last_kmer': True, 'support': sup}))
    out.append(Case(planted(n, at=200 - n - 50)[:199], {'last_kmer': False, 'support': sup - 1}))
    return out


# ----------------------------------------------------------------------------------------------------------------------------
# 4. plateaus: an exact repeat of p has s[d] equal on [p-3, p+3]; placed over lanes 63|64 (one wave: a stride wrap; four waves: the
#    boundary of two waves) and over threads 255|256 (four waves: a stride wrap)
# ----------------------------------------------------------------------------------------------------------------------------
def plateau_periods(K):
    """p with (p - 3 - DMIN) % 64 == 61, four of them: the plateau lies over the boundaries of waves 0|1, 1|2, 2|3 and over the wrap 255|0"""
    first = K['CCS_DMIN'] + K['CCS_SMOOTH'] + 61
    return [first + 64 * j for j in range(4)]


def plateaus(K):
    out = []
    for p in plateau_periods(K):
        u = unit_of(p, 'plateau')
        for L in (2 * p + 10, 2 * p + p // 2 + 1, 3 * p + 17):
            lo = p - K['CCS_SMOOTH'] - K['CCS_DMIN']
            out.append(Case(tandem(u, L), {'unit': p, 'length': L, 'lanes64': [(lo + t) % 64 for t in range(7)],
                                           'lanes256': [(lo + t) % 256 for t in range(7)]}))
    return out


# ----------------------------------------------------------------------------------------------------------------------------
# 5. harmonics
# ----------------------------------------------------------------------------------------------------------------------------
def alternating(p, pairs, subs, more, trim, *key):
    """A B A B ..: B is A with `subs` evenly spaced substitutions; the last `more` B copies carry one more, half a step on; `trim` bases
    are cut off the end"""
    a = unit_of(p, 'harmonic', *key)
    step = p // (subs + 1)
    at = [step * (j + 1) - 1 for j in range(subs)]
    b, b1 = substitute(a, at), substitute(a, at + [step // 2])
    copies = []
    for j in range(pairs):
        copies += [a, b1 if j >= pairs - more else b]
    read = np.concatenate(copies)
    return read[:len(read) - trim].copy()


# (subs, more, trim, margin of q = 2) picked from search_harmonics(): the smallest margin at which the fundamental is taken and the
# largest at which it is not
HARMONIC_TUNED = ((4, 2, 3, 0), (4, 2, 4, -1))


def search_harmonics(p=60, pairs=4):
    """margin 2 s[e] - best of q = 2 -> (subs, more, trim), over the grid the cases are picked from (run on the CPU; see harmonics())"""
    import oracle_lib
    found = {}
    for subs in (3, 4, 5):
        for more in range(0, pairs + 1):
            for trim in range(0, 50):
                t = oracle_lib.oracle_ccs_trace(alternating(p, pairs, subs, more, trim))
                h = [x for x in t['harmonics'] if x['q'] == 2]
                if h and t['bestd'] > 2 * p - 4:
                    found.setdefault(h[0]['margin'], (subs, more, trim))
    return found


def harmonics(K):
    out = [Case(alternating(60, 4, s, pa, tr), {'q': 2, 'margin': m}) for s, pa, tr, m in HARMONIC_TUNED]
    # A B C A B C ..: neighbours share little, copies three apart everything; 2p / 3 is no period, p is
    a = unit_of(60, 'three')
    b, c = substitute(a, range(5, 60, 20)), substitute(a, range(12, 60, 20))
    out.append(Case(np.concatenate([a, b, c] * 3 + [a]), {'q': 3, 'wins': True}))
    # bestd 97: q = 2 and 3 are evaluated, q = 4 gives 24 < CCS_DMIN and ends the loop
    out.append(Case(tandem(unit_of(100, 'break'), 520), {'evaluated': 2}))
    return out


# ----------------------------------------------------------------------------------------------------------------------------
# 6. cuts and caps
# ----------------------------------------------------------------------------------------------------------------------------
def cuts(K):
    cap, tail = K['CCS_MAX_CUTS'], K['CCS_MIN_TAIL']
    u = unit_of(40, 'cap')
    out = [Case(tandem(u, 40 * n), {'copies': n, 'ncuts': min(n, cap), 'tail': False}) for n in (cap - 1, cap, cap + 1)]
    out += [Case(tandem(u, 40 * (cap - 1) + tail - 1), {'copies': cap - 1, 'ncuts': cap - 1, 'tail': False}),
            Case(tandem(u, 40 * (cap - 1) + tail), {'copies': cap - 1, 'ncuts': cap - 1, 'tail': True}),
            Case(tandem(u, 40 * cap + tail), {'copies': cap, 'ncuts': cap, 'tail': False})]        # long enough, but behind the cap
    for p in (42, 43):                   # p0 = p - 3 = 39, 40: tol 4 and 5
        out.append(Case(tandem(unit_of(p, 'tol'), 6 * p + 7), {'p0': p - 3, 'tol': max(4, (p - 3) // 8)}))
    for p in (98, 99, 100):              # p0 = 95, 96, 97: W = p0, 96, 96
        out.append(Case(tandem(unit_of(p, 'W'), 5 * p + 30), {'p0': p - 3, 'W': min(p - 3, 96)}))
    u = unit_of(100, 'last cut')         # p0 97, tol 12, dlo 85
    out += [Case(tandem(u, 385), {'last': 85, 'ncuts': 4}), Case(tandem(u, 384), {'last': 84, 'ncuts': 3, 'tail': True})]
    return out


# ----------------------------------------------------------------------------------------------------------------------------
# 7. the vote: ties of two offsets, a window without a valid k-mer, a recurrence beyond the guard
# ----------------------------------------------------------------------------------------------------------------------------
def delete(read, at, n=1):
    return np.concatenate([read[:at], read[at + n:]])


# positions found by a search over the deleted base with the oracle's trace (tests/test_ccs_edges_host.py states what they reach)
VOTE_BY_DISTANCE = 202          # one base gone: cut 2 has as many anchors at 99 as at 100; prev = 100 takes 100, the larger
VOTE_BY_DISTANCE_FIRST = 151    # the same at cut 0, where prev = p0 = 97 takes 99
VOTE_BY_DELTA = (153, 227)      # one base gone, then two: cut 2 has as many anchors at 98 as at 100 and prev = 99 lies between


def vote(K):
    p = 100                      # p0 97, tol 12 > CCS_GUARD, W 96
    base = tandem(unit_of(p, 'vote'), 650)
    out = [Case(delete(base, VOTE_BY_DISTANCE), {'tie': 'distance', 'cut': 2, 'between': (99, 100), 'v': 100}),
           Case(delete(base, VOTE_BY_DISTANCE_FIRST), {'tie': 'distance', 'cut': 0, 'between': (99, 100), 'v': 99}),
           Case(delete(delete(base, VOTE_BY_DELTA[0]), VOTE_BY_DELTA[1], 2), {'tie': 'delta', 'cut': 2, 'between': (98, 100), 'v': 98})]
    # N every 8 bases over the windows of the cuts at 200 and 300: no valid k-mer, no anchor, the cut is the candidate nearest prev
    masked = base.copy()
    masked[200 - 96 - 7:300 + 96 + 8:8] = 4
    out.append(Case(masked, {'no_anchor': (2, 3)}))
    # the 8-mer centred on the cut at 200 occurs again 109 later, 9 from the vote and inside the tolerance; the true recurrences of the
    # nine k-mers nearest the cut are gone (two substitutions in the partner copy), so only the guard keeps the cut from following it
    b = 200
    far = substitute(base, [b + p - 1, b + p])
    far[b - 4 + p + 9:b + 4 + p + 9] = far[b - 4:b + 4]
    out.append(Case(far, {'beyond_guard': 2, 'dist': 5}))
    return out


# ----------------------------------------------------------------------------------------------------------------------------
# 8. the anchor's keys
# ----------------------------------------------------------------------------------------------------------------------------
def anchor_keys(K):
    # keys 1 and 2: in the partner copy of the cut at 200 the base at b + p is gone and the one before it is another: the anchors nearest
    # the cut start at b - 9 (offset p) and b + 1 (offset p - 1), both 5 from it; the larger i wins and the cut moves by one base
    p, b = 100, 200
    base = tandem(unit_of(p, 'anchor'), 650)
    out = [Case(delete(substitute(base, [b + p - 1]), b + p), {'key': 2, 'cut': 2, 'dist': 5, 'i': b + 1, 'delta': p - 1})]
    # keys 3 and 4: the 8-mer centred on every copy boundary is a stretch of period 5; around the boundary at 3p the stretch is 18 bases,
    # so the anchor at 2p - 4 recurs at p - 5, p and p + 5 (prev = p takes p), and at p - 5 and p + 5 alone once offset 3 of the middle
    # recurrence is substituted (equal distance from prev: the smaller)
    p = 80                       # p0 77, tol 9: p - 5 and p + 5 are candidates, and within CCS_GUARD of the vote
    u = unit_of(p, 'anchor keys')
    pat = np.array([0, 1, 3, 2, 1], dtype=np.int8)
    for j in range(-4, 4):
        u[j % p] = pat[j % 5]
    base = tandem(u, 7 * p + 20)
    for j in range(-9, 9):
        base[3 * p + j] = pat[j % 5]
    out.append(Case(base.copy(), {'key': 3, 'cut': 2, 'i': 2 * p - 4, 'delta': p, 'tied': 3}))
    out.append(Case(substitute(base, [3 * p - 1]), {'key': 4, 'cut': 2, 'i': 2 * p - 4, 'delta': p - 5, 'tied': 2}))
    return out


# ----------------------------------------------------------------------------------------------------------------------------
# 9. N and odd codes (hip.pack hands any int8 through: 7 and -3 reach the kernel, which reads them as "not 0..3" like the oracle)
# ----------------------------------------------------------------------------------------------------------------------------
def n_codes(K):
    u = unit_of(90, 'N')
    base = tandem(u, 5 * 90 + 33)
    first_last = base.copy()
    first_last[0] = first_last[-1] = 4
    masked = base.copy()
    masked[180:270:8] = 4                 # no valid 8-mer starts in the third copy
    odd = base.copy()
    odd[100], odd[291] = 7, -3
    return [Case(first_last, {'N': 'first and last'}), Case(masked, {'N': 'every 8th of a copy', 'copy': (180, 270)}),
            Case(np.full(300, 4, dtype=np.int8), {'N': 'all', 'period': 0}), Case(odd, {'odd': (100, 291)})]


# ----------------------------------------------------------------------------------------------------------------------------
# 10. chains: every position in one, two, three chains; many codes in few buckets
# ----------------------------------------------------------------------------------------------------------------------------
LOW_COMPLEXITY = 1100


def few_buckets(K, nbuckets=512):
    """runs of four equal letters: among 40 seeds the read whose distinct 8-mers use the fewest buckets per code"""
    best = None
    for seed in range(40):
        rng = _rng('runs', seed)
        r = np.repeat(np.array([rng.randrange(4) for _ in range(LOW_COMPLEXITY // 4)], dtype=np.int8), 4)
        codes = set()
        for i in range(len(r) - 7):
            c = 0
            for b in r[i:i + 8]:
                c = (c << 2) | int(b)
            codes.add(c)
        ratio = len({(c ^ (c >> 5)) & (nbuckets - 1) for c in codes}) / float(len(codes))
        if best is None or ratio < best[0]:
            best = (ratio, r)
    return best[1]


def chains(K):
    L = LOW_COMPLEXITY
    return [Case(np.zeros(L, dtype=np.int8), {'chains': 1}), Case(tandem(np.array([0, 2], dtype=np.int8), L), {'chains': 2}),
            Case(tandem(np.array([1, 3, 0], dtype=np.int8), L), {'chains': 3}), Case(few_buckets(K), {'few_buckets': True})]


SETS = collections.OrderedDict([('classes', classes), ('thresholds', thresholds), ('period limits', period_limits), ('plateaus', plateaus),
                                ('harmonics', harmonics), ('cuts', cuts), ('vote', vote), ('anchor keys', anchor_keys),
                                ('N and odd codes', n_codes), ('chains', chains)])


# ----------------------------------------------------------------------------------------------------------------------------
# expected values: clo_ccs_segments plus the tail rule of poa_kernel_body, and oracle_find_consensus; computed once and shared
# ----------------------------------------------------------------------------------------------------------------------------
_want = {}


def want_of(read, K):
    """{'period', 'segs' [(start, end)], 'consensus' (segments, ccs) | (None, None)} of the oracle for a read"""
    import oracle_lib
    key = read.tobytes()
    if key not in _want:
        period, cut_at, _support = oracle_lib.oracle_ccs_segments(read)
        segs, b = [], 0
        for c in cut_at:
            segs.append((b, c))
            b = c
        if period and len(read) - b >= K['CCS_MIN_TAIL'] and len(cut_at) < K['CCS_MAX_CUTS']:
            segs.append((b, len(read)))
        _want[key] = {'period': period, 'segs': segs, 'consensus': tuple(oracle_lib.oracle_find_consensus(read)[:2])}
    return _want[key]


def filler(K, L):
    """an ordinary read of exactly L bases (a repeat of period 150 with a few substitutions): pads a batch to a launch class"""
    r = tandem(unit_of(150, 'filler'), L)
    return substitute(r, range(40, L, 97))
