"""Seeded Smith-Waterman cases over substitution matrices of 6..32 letters (K1a, csrc/ssw_alpha.hip) at the edges where that path is
most likely to be wrong: asymmetric matrices (a transposed lookup changes answers), the read-length buckets of the LDS form and the
global form above 8 192 rows, the switch from the 8-bit to the 16-bit pass, the 16-bit ceiling, the traceback's windows (ring, band,
staged sequences, the stated CIGAR_TRUNC condition) and the gap costs.  The reference's answers live in
tests/golden/ssw_alphabet_edges_golden.json.gz (made by tests/golden/make_ssw_alphabet_edges_golden.py from oracle/_ref/libssw.so);
tests/test_ssw_alphabet_edges_host.py holds the CPU statement to them and tests/test_gpu_ssw_alphabet_edges.py the kernels.  The batches
too large for a golden file (more global-form tasks than workgroups, traceback pool pressure) are made here as well and checked against
the CPU oracle only.

A case is (reference, read, matrix, keyword arguments of oracle_align / ref_align): the sequences are strings over LETTERS (code k is
LETTERS[k]), the matrix a flat n * n list, row = reference code."""
import json
import zlib

import numpy as np

GOLDEN_NAME = 'ssw_alphabet_edges_golden.json.gz'
LETTERS = 'ABCDEFGHIJKLMNOPQRSTUVWXYZabcdef'

# the read-length buckets of K1a (csrc/clh_device.h kAlphaRows) and reads around each boundary
ALPHA_ROWS = (256, 1024, 4096, 8192)
BUCKET_LENGTHS = (1, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193, 12000, 20000)
# the traceback's windows (ssw_traceback.hip launch_ssw_alpha_traceback): the small attempt has 514 rows of state, a ring of 512 when
# w + 3 <= 512, sequences in LDS up to 6 144 bytes; the big launch for a class whose longest read is >= 5 120 rows has 5 122 rows, a ring
# of 4 096 and 153 600 - 28 * 5 122 = 10 184 bytes of sequence
SMALL_WS, SMALL_RING, SMALL_SEQ = 514, 512, 6144
BIG_WS, BIG_RING, BIG_SEQ = 5122, 4096, 153600 - 28 * 5122


def _s(codes):
    return ''.join(LETTERS[int(c)] for c in codes)


_LUT = np.full(256, -1, dtype=np.int16)
for _i, _c in enumerate(LETTERS):
    _LUT[ord(_c)] = _i


def decode(s):
    """letters -> int8 codes"""
    return _LUT[np.frombuffer(s.encode('latin-1'), dtype=np.uint8)].astype(np.int8)


def mutate(rng, s, n, p, letters=None):
    """substitutions / insertions of 1..5 letters / deletions at rate p (a third each); letters: the codes to draw from"""
    pool = np.arange(n) if letters is None else np.asarray(letters)
    out = []
    for c in s:
        u = rng.random()
        if u < p / 3:
            continue
        if u < 2 * p / 3:
            out.append(int(rng.choice(pool))); continue
        out.append(int(c))
        if u < p:
            out.extend(int(x) for x in rng.choice(pool, int(rng.integers(1, 6))))
    return np.array(out if out else [int(pool[0])], dtype=np.int8)


def blosum62():
    from ciri_long_amd.ssw_wrap import BLOSUM62
    return [int(x) for x in BLOSUM62.astype(np.int8).reshape(-1)]


def asym_matrix(rng, n, dead_rows=(), dead_cols=()):
    """an asymmetric n x n matrix: every entry drawn on its own (mat[a][b] and mat[b][a] differ in sign and size for many pairs), a
    positive diagonal; the rows in dead_rows (reference letters) and the columns in dead_cols (read letters) all negative"""
    m = rng.integers(-9, 7, size=(n, n))
    np.fill_diagonal(m, rng.integers(2, 12, size=n))
    for r in dead_rows:
        m[r, :] = rng.integers(-9, 0, size=n)
    for c in dead_cols:
        m[:, c] = rng.integers(-9, 0, size=n)
    return [int(x) for x in m.astype(np.int8).reshape(-1)]


def diag_matrix(rng, n, diag, lo, hi=0):
    """diagonal `diag` (one entry per letter), off-diagonal entries in [lo, hi] with lo itself present: a read that copies a piece of the
    reference scores exactly the sum of its letters' diagonal entries, nothing scores more"""
    m = rng.integers(lo, hi + 1, size=(n, n))
    m[0, 1] = lo
    np.fill_diagonal(m, diag)
    return [int(x) for x in m.astype(np.int8).reshape(-1)]


def read_with_score(rng, diag, S, L):
    """L letters whose diagonal entries sum to S (the diagonal holds its maximum minus 1; see cut_diagonal)"""
    diag = np.asarray(diag)
    dmax = int(diag.max())
    top = np.flatnonzero(diag == dmax)
    q = rng.choice(top, L).astype(np.int8)
    excess = L * dmax - S
    assert 0 <= excess <= L * (dmax - int(diag.min())), (S, L)
    for p in rng.permutation(L):
        if excess == 0:
            break
        want = int(diag[diag >= dmax - excess].min())          # the largest cut that does not overshoot
        q[p] = int(rng.choice(np.flatnonzero(diag == want))); excess -= dmax - want
    assert excess == 0 and int(diag[q.astype(np.int64)].sum()) == S
    return q


def cut_diagonal(rng, n, hi):
    """a diagonal for read_with_score: letter 0 scores hi, letters 1 and 2 score 1, the next ones hi - 1, hi - 2, hi - 4, ... (any cut below
    hi takes a few letters), the rest random in 1..hi"""
    special = [hi, 1, 1] + [hi - c for c in (1, 2, 4, 8, 16, 32, 64) if hi - c > 1]
    assert len(special) <= n
    return np.concatenate([special, rng.integers(1, hi + 1, n - len(special))]).astype(np.int64)


def read_summing_to(rng, diag, S, min_len=1):
    """random letters, each drawn from those whose diagonal entry fits what is left of S, until their diagonal entries sum to S"""
    diag = np.asarray(diag)
    while True:
        q, rem = [], S
        while rem > 0:
            c = int(rng.choice(np.flatnonzero(diag <= rem)))
            q.append(c); rem -= int(diag[c])
        if len(q) >= min_len:
            return np.array(q, dtype=np.int8)


def diag_of(mat):
    n = int(round(len(mat) ** 0.5))
    return [mat[k * n + k] for k in range(n)]


def _kw(gap_open, gap_extend, flag=1, score_size=2, maskl=None, filters=0, filterd=0):
    kw = dict(gap_open=gap_open, gap_extend=gap_extend, flag=flag, score_size=score_size, filters=filters, filterd=filterd)
    if maskl is not None:
        kw['maskl'] = maskl
    return kw


def _planted(rng, n, read, left, right, letters=None):
    """a reference: `left` and `right` random letters around the read"""
    pool = np.arange(n) if letters is None else np.asarray(letters)
    return np.concatenate([rng.choice(pool, left).astype(np.int8), read, rng.choice(pool, right).astype(np.int8)])


# ---- the sets ----------------------------------------------------------------------------------------------------------------------
def asymmetric():
    """asymmetric matrices of edge 6, 20, 24, 32 with all-negative rows and columns; related and unrelated pairs, reads that hold
    letters the reference lacks and references that hold letters the read lacks"""
    rng = np.random.default_rng(6203)
    cases = []
    for n in (6, 20, 24, 32):
        mat = asym_matrix(rng, n, dead_rows=(n - 1,), dead_cols=(n - 2,))
        half = list(range(n // 2)); other = list(range(n // 2, n))
        for k in range(14):
            L = int(rng.choice([8, 40, 150, 400]))
            if k % 7 == 0:                                      # unrelated
                read = rng.integers(0, n, L).astype(np.int8)
                ref = rng.integers(0, n, int(rng.integers(20, 600))).astype(np.int8)
            elif k % 7 == 1:                                    # the read holds letters the reference lacks
                core = rng.choice(half, L).astype(np.int8)
                read = mutate(rng, core, n, 0.2, letters=other)
                ref = _planted(rng, n, core, int(rng.integers(0, 200)), 30, letters=half)
            elif k % 7 == 2:                                    # the reference holds letters the read lacks
                read = rng.choice(half, L).astype(np.int8)
                ref = _planted(rng, n, mutate(rng, read, n, 0.2, letters=other), 50, int(rng.integers(0, 200)), letters=other)
            else:                                               # mutated copies
                core = rng.integers(0, n, L).astype(np.int8)
                read = mutate(rng, core, n, float(rng.choice([0.05, 0.15, 0.3])))
                ref = _planted(rng, n, core, int(rng.integers(0, 300)), int(rng.integers(0, 100)))
            go = int(rng.integers(1, 12)); ge = int(rng.integers(0, go + 1))
            cases.append((_s(ref), _s(read), mat, _kw(go, ge, flag=int(rng.choice([1, 1, 15])), score_size=int(rng.choice([2, 2, 1, 0])),
                                                       maskl=max(15, len(read) // 2))))
    return cases


def buckets():
    """reads at and around the bucket boundaries of K1a, the global form's 8 193 rows and more: mutated copies and unrelated pairs, all
    of one matrix and option set, so that a batch holds every length and one segment's longest read sizes the LDS for the others"""
    rng = np.random.default_rng(8192)
    cases = []
    for mat in (blosum62(), asym_matrix(rng, 32)):
        n = int(round(len(mat) ** 0.5))
        for L in BUCKET_LENGTHS:
            core = rng.integers(0, n, L).astype(np.int8)
            rate = 0.0 if L < 300 else 0.03
            read = mutate(rng, core, n, rate)[:L] if rate else core.copy()
            if len(read) < L:
                read = np.concatenate([read, rng.integers(0, n, L - len(read)).astype(np.int8)])
            ref = _planted(rng, n, core, int(rng.integers(0, 300)), 40)
            cases.append((_s(ref), _s(read), mat, _kw(11, 1)))
            unrel = rng.integers(0, n, L).astype(np.int8)               # unrelated, against a short reference
            cases.append((_s(rng.integers(0, n, int(rng.integers(30, 200))).astype(np.int8)), _s(unrel), mat, _kw(11, 1)))
    return cases


def threshold():
    """exact and near-exact copies whose best score plus bias is 253, 254, 255, 256 (the 8-bit pass overflows at 255), score_size
    0 / 1 / 2, matrices whose minimum is -1, -6, -128 and whose maximum is 11 or 127"""
    rng = np.random.default_rng(255)
    cases = []
    for lo, hi, n in ((-1, 11, 8), (-6, 11, 20), (-128, 11, 32), (-1, 127, 24), (-6, 127, 20), (-128, 127, 32)):
        diag = cut_diagonal(rng, n, hi)
        m = np.array(diag_matrix(rng, n, diag, lo, 0)).reshape(n, n)
        m[1, 2] = -1                                        # reference letter 1 against read letter 2: the near copies' substitution
        mat = [int(x) for x in m.reshape(-1)]
        bias = -lo
        for target in (253, 254, 255, 256):
            S = target - bias
            for near in (False, True):
                if near:                                    # letter 1 (diagonal 1) in the middle of the reference copy, letter 2 (also 1)
                    rest = read_summing_to(rng, diag, S + 1, 2)       # in the read, scored -1: the full path scores S
                    p = len(rest) // 2
                    refcore = np.concatenate([rest[:p], [1], rest[p:]]).astype(np.int8)
                    read = refcore.copy(); read[p] = 2
                else:
                    read = read_summing_to(rng, diag, S)
                    refcore = read.copy()
                ref = _planted(rng, n, refcore, int(rng.integers(5, 120)), int(rng.integers(5, 60)))
                for score_size in (0, 1, 2):
                    cases.append((_s(ref), _s(read), mat, _kw(int(rng.integers(3, 12)), 1, score_size=score_size)))
    return cases


def ceiling():
    """scores of 32 766, 32 767, just above it and far above it: a diagonal of 127 (reads of ~258 letters, LDS form), BLOSUM62 W-W
    (~2 979 letters), a diagonal of 4 (~8 193 letters, global form); mutated variants; a saturating copy placed twice in the
    reference, so that the first column that reaches 32 767 decides ref_begin"""
    rng = np.random.default_rng(32767)
    cases = []
    # a diagonal of 127 (and the cuts of cut_diagonal), off-diagonal -6..0
    n = 20
    diag = cut_diagonal(rng, n, 127)
    m127 = diag_matrix(rng, n, diag, -6, 0)
    for S, L in ((32766, 258), (32767, 259), (32768, 260), (32770, 262), (32766, 400), (32767, 300), (40000, 330), (127 * 1000, 1000)):
        read = read_with_score(rng, diag, S, L)
        for variant in ('copy', 'mutated', 'twice'):
            if variant == 'copy':
                ref = _planted(rng, n, read, int(rng.integers(3, 80)), int(rng.integers(3, 40)))
                q = read
            elif variant == 'mutated':
                ref = _planted(rng, n, read, int(rng.integers(3, 80)), int(rng.integers(3, 40)))
                q = mutate(rng, read, n, 0.01)
            else:
                ref = np.concatenate([_planted(rng, n, read, 20, 50), read, rng.integers(0, n, 10).astype(np.int8)])
                q = read
            for score_size, flag in ((2, 1), (1, 15)):
                cases.append((_s(ref), _s(q), m127, _kw(6, 1, flag=flag, score_size=score_size)))
    # BLOSUM62: W-W is 11, 2 979 W reach 32 769; reads of mostly W, copies, mutated, twice
    b = blosum62()
    W = 17
    for L, wfrac, variant in ((2978, 1.0, 'copy'), (2979, 1.0, 'copy'), (2979, 1.0, 'twice'), (3100, 0.97, 'copy'), (3300, 0.9, 'mutated'),
                              (3000, 0.99, 'mutated'), (3600, 0.8, 'copy')):
        read = np.where(rng.random(L) < wfrac, W, rng.integers(0, 20, L)).astype(np.int8)
        if variant == 'twice':
            ref = np.concatenate([rng.integers(0, 20, 30), read, rng.integers(0, 20, 40), read, rng.integers(0, 20, 5)]).astype(np.int8)
        else:
            ref = _planted(rng, 20, read, int(rng.integers(5, 100)), 30)
        q = mutate(rng, read, 20, 0.01) if variant == 'mutated' else read
        cases.append((_s(ref), _s(q), b, _kw(11, 1, flag=1, score_size=2)))
    # a diagonal of 4 (and 3, 2, 1 for a few letters): the global form at the ceiling
    n = 24
    diag4 = np.concatenate([[4, 3, 1, 2], np.full(n - 4, 4)])
    m4 = diag_matrix(rng, n, diag4, -3, 0)
    for S, L, variant in ((32766, 8200, 'copy'), (32767, 8194, 'copy'), (32768, 8193, 'copy'), (32767, 8300, 'twice'), (34000, 8600, 'mutated')):
        read = read_with_score(rng, diag4, S, L)
        if variant == 'twice':
            ref = np.concatenate([rng.integers(0, n, 10), read, rng.integers(0, n, 30), read]).astype(np.int8)
        else:
            ref = _planted(rng, n, read, 40, 20)
        q = mutate(rng, read, n, 0.002) if variant == 'mutated' else read
        cases.append((_s(ref), _s(q), m4, _kw(5, 2, flag=1, score_size=2)))
    return cases


def _gapped(rng, n, pieces, gaps, mat_letters=None):
    """a read made of exact copies of reference pieces of the lengths in `pieces`, the reference skipping gaps[k] letters between piece
    k and k + 1 (a negative gap: the read repeats -gaps[k] letters of the reference, an insertion)"""
    pool = np.arange(n) if mat_letters is None else np.asarray(mat_letters)
    total = sum(pieces) + sum(max(0, g) for g in gaps) + 10
    body = rng.choice(pool, total).astype(np.int8)
    read, pos = [], 0
    for k, P in enumerate(pieces):
        read.append(body[pos:pos + P]); pos += P
        if k < len(gaps):
            g = gaps[k]
            if g >= 0:
                pos += g
            else:
                read.append(rng.choice(pool, -g).astype(np.int8))
    ref = body[:pos]
    return np.concatenate(read).astype(np.int8), ref


def windows():
    """insertions and deletions sized so that the band (|aligned reference - aligned read| + 1, doubled while the walk leaves it) sits
    at the small attempt's ring limit (509 / 510 / 511) with aligned reads below and above its 514 rows, at the big launch's ring limit
    (4 093 / 4 094), and read + reference at the small attempt's 6 144 bytes and the big launch's 10 184; mutated and multi-iteration
    alignments in the unstaged path; a few that meet the stated CIGAR_TRUNC condition (aligned read over 5 121 rows, band over 4 093).
    One matrix (diagonal 3..5, asymmetric off-diagonal -5..1) and one option set: the batch's classes are those the GPU test asserts."""
    rng = np.random.default_rng(5122)
    n = 24
    m = rng.integers(-5, 2, size=(n, n))
    np.fill_diagonal(m, rng.integers(3, 6, size=n))
    mat = [int(x) for x in m.astype(np.int8).reshape(-1)]
    cases = []

    def add(pieces, gaps, rate=0.0, lead=20, tail=20):
        read, body = _gapped(rng, n, pieces, gaps)
        if rate:
            read = mutate(rng, read, n, rate)
        ref = np.concatenate([rng.integers(0, n, lead), body, rng.integers(0, n, tail)]).astype(np.int8)
        cases.append((_s(ref), _s(read), mat, _kw(6, 1)))

    for w in (509, 510, 511):                           # the small attempt's ring, aligned reads of 400 (fit 514 rows) and 600 (do not)
        add([200, 200], [w - 1])
        add([300, 300], [w - 1])
    add([128, 127, 300], [300, -46])                    # band 255 -> 510 after one doubling (the walk leaves the first band)
    add([1500, 1400], [3244 - 2900])                    # read + reference 6 144 (band 345: small attempt, staged)
    add([1500, 1400], [3245 - 2900])                    # 6 145: the big launch
    add([2500, 2500], [5184 - 5000])                    # 10 184 (class -13, longest read >= 5 120 rows: staged in the big launch)
    add([2500, 2500], [5185 - 5000])                    # 10 185: unstaged
    for w in (4093, 4094):                              # the big launch's ring
        add([2500, 2500], [w - 1])
    add([2000, 1000, 2500], [600, -200], rate=0.01)     # unstaged, mutated, the walk leaves the first band (multi-iteration)
    add([3000, 2900], [900], rate=0.02)                 # unstaged, mutated
    add([2600, 2700], [4300], lead=10, tail=10)         # the stated CIGAR_TRUNC condition: 5 300 rows, band 4 301
    add([3000, 2600], [4200], rate=0.005)
    add([5300], [], lead=1, tail=1)                     # a long read in the class (sizes the big launch at 5 122 rows)
    return cases


def gap_costs():
    """gap_open 255, gap_extend 0, gap_open == gap_extend with scores past the 8-bit pass, a large gap_extend; each with flag 0 / 1 / 15
    and maskLen below and above 15"""
    rng = np.random.default_rng(2550)
    cases = []
    b = blosum62()
    for go, ge in ((255, 0), (255, 1), (255, 255), (11, 0), (1, 0), (3, 3), (7, 7), (120, 100)):
        for flag in (0, 1, 15):
            for k, L in enumerate((60, 300, 1200)):
                core = rng.integers(0, 20, L).astype(np.int8)
                read = core.copy()
                for _ in range(int(rng.integers(1, 4))):     # indels the gap terms decide
                    p = int(rng.integers(5, len(read) - 5))
                    read = np.concatenate([read[:p], rng.integers(0, 20, int(rng.integers(1, 12))).astype(np.int8), read[p:]]) \
                        if rng.random() < 0.5 else np.concatenate([read[:p], read[p + int(rng.integers(1, 12)):]])
                read = mutate(rng, read, 20, 0.05)
                ref = _planted(rng, 20, core, int(rng.integers(0, 200)), 40)
                maskl = (int(rng.integers(1, 15)), max(15, len(read) // 2))[k & 1]
                cases.append((_s(ref), _s(read), b, _kw(go, ge, flag=flag, maskl=maskl, filters=int(rng.choice([0, 100])),
                                                         filterd=int(rng.choice([0, 50, 10000])))))
    return cases


def all_cases():
    """every golden case set by its key in the golden file"""
    return {
        'asymmetric': asymmetric(),
        'buckets': buckets(),
        '8-bit threshold': threshold(),
        'ceiling': ceiling(),
        'traceback windows': windows(),
        'gap costs': gap_costs(),
    }


def case_crc(case):
    ref, q, mat, kw = case
    return zlib.crc32(json.dumps([ref, q, list(mat), sorted(kw.items())]).encode()) & 0xffffffff


def call_args(case):
    """(ref, read) as int8 codes and keyword arguments for oracle_align / ref_align"""
    ref, q, mat, kw = case
    kw = dict(kw)
    kw['mat'] = np.asarray(mat, dtype=np.int8)
    return (decode(ref), decode(q)), kw


# ---- batches checked against the CPU oracle only -------------------------------------------------------------------------------------
def global_many(n_cu, seed=8193):
    """more alignments above 8 192 rows than the global form has workgroups (n_cu * 8): n_cu * 8 + 100 reads of 8 193..9 700 letters
    (varied, so that a stale slot of a longer earlier task would show) against references of 50..150 letters, a mutated piece of each
    reference planted in most reads"""
    rng = np.random.default_rng(seed)
    n = 20
    mat = asym_matrix(rng, n)
    refs, reads = [], []
    for k in range(n_cu * 8 + 100):
        R = int(rng.integers(50, 151))
        ref = rng.integers(0, n, R).astype(np.int8)
        L = int(rng.integers(8193, 9701))
        read = rng.integers(0, n, L).astype(np.int8)
        if k % 4:
            core = mutate(rng, ref, n, 0.1)[:L]
            a = int(rng.integers(0, L - len(core) + 1))
            read[a:a + len(core)] = core
        refs.append(ref); reads.append(read)
    return refs, reads, mat


def pool_pressure(count=450, seed=4000):
    """BLOSUM62 pairs whose alignment skips 2 000 reference letters: a 1 000-letter read, its halves mutated copies of the first and
    the last 500 letters of a 3 000-letter reference.  Each traceback keeps about 4 MB of direction bytes (one per band cell)"""
    rng = np.random.default_rng(seed)
    refs, reads = [], []
    for _ in range(count):
        ref = rng.integers(0, 20, 3000).astype(np.int8)
        read = np.concatenate([mutate(rng, ref[:500], 20, 0.05), mutate(rng, ref[2500:], 20, 0.05)])
        refs.append(ref); reads.append(read)
    return refs, reads
