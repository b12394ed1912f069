"""Seeded cases for the end-anchored alignment kernels (K1g, csrc/ssw_ends.hip) at the edges where they are most likely to be wrong
(not a test module): asymmetric matrices (a transposed lookup changes answers), queries around the 64-row blocks, references around
the lane, register and nibble that own column n, the overlap mode's end-cell rules at exact ties, gap costs under which almost every
cell is a tie, the int32 frame at the real chunk width, CIGARs with as many runs as the host reserves, and batches the workspace cuts
into shares.  Every expected value is tests/ends_check.py; tests/test_ends_edges_host.py proves that the sets reach what they are
named for and holds tools/ends_model.py to them, tests/test_gpu_ends_edges.py holds the kernels to them.

A case is Case(ref, query, scoring, alphabet, go, ge, mode): the sequences are strings, `scoring` is (match, mismatch) with
alphabet None (DNA, codes of 'ACGTN') or an n x n int64 matrix (row = reference letter) over `alphabet`.  Lengths come from `geom`,
{'cpl': reference columns a lane owns, 'chunk': columns of a chunk} -- EndsPlan.info() on the device, {'cpl': 8, 'chunk': 512} here."""
import collections

import numpy as np

import ends_check as chk

MODES = chk.MODES
HOST_GEOM = {'cpl': 8, 'chunk': 512}
LETTERS = 'ABCDEFGHIJKLMNOPQRSTUVWXYZ234567'
OVERLAP_SCORING = (1, 3, 5, 2)          # unrelated flanks lose: a shared piece alone is best

Case = collections.namedtuple('Case', 'ref query scoring alphabet go ge mode')


def matrix_of(case):
    """the checker's matrix (int64, mat[reference code][query code])"""
    return chk.dna_matrix(*case.scoring) if case.alphabet is None else np.asarray(case.scoring, dtype=np.int64)


def codes_of(case):
    """-> (query codes, reference codes)"""
    alpha = 'ACGTN' if case.alphabet is None else case.alphabet
    return chk.encode(case.query, alpha), chk.encode(case.ref, alpha)


def expected(case, path=True):
    q, r = codes_of(case)
    return chk.align(q, r, matrix_of(case), case.go, case.ge, case.mode, path=path)


def scoring_key(case):
    """cases with the same key go to the device in one call"""
    s = case.scoring if case.alphabet is None else np.asarray(case.scoring, dtype=np.int64).tobytes()
    return (s, case.alphabet, case.go, case.ge, case.mode)


def _modes(pairs, scoring, alphabet, go, ge, modes=MODES):
    return [Case(r, q, scoring, alphabet, go, ge, mode) for mode in modes for r, q in pairs]


def _copy(rng, ref, a, m, alpha, rate=0.10):
    """a noisy copy of ref[a:a + m], exactly m letters (filled up with unrelated ones)"""
    return (chk.mutate(rng, ref[a:a + m], rate, alpha) + chk.random_seq(rng, m, alpha))[:m]


# ------------------------------------------------------------------------------------------------------------------------------
# asymmetric: smat[query code][reference code] is filled from mat[rc * n_mat + qc]; only an asymmetric matrix tells the two apart
# ------------------------------------------------------------------------------------------------------------------------------
def asymmetric_matrices():
    """-> [(name, matrix)]: edges 2, 5, 20, 32 with every entry drawn in -9..9, and one of edge 5 that holds -128 and 127"""
    out = []
    for n in (2, 5, 20, 32):
        rng = chk.rng_for('edges asymmetric matrix', n)
        while True:
            mat = np.array([[rng.randint(-9, 9) for _ in range(n)] for _ in range(n)], dtype=np.int64)
            if (mat != mat.T).any():
                break
        out.append(('edge %d' % n, mat))
    rng = chk.rng_for('edges asymmetric matrix', 'int8 limits')
    mat = np.array([[rng.randint(-9, 9) for _ in range(5)] for _ in range(5)], dtype=np.int64)
    mat[0, 1], mat[1, 0], mat[3, 2], mat[2, 3], mat[4, 4], mat[2, 2] = -128, 127, -128, 5, 127, 127
    out.append(('int8 limits', mat))
    return out


def asymmetric(geom):
    cases = []
    for name, mat in asymmetric_matrices():
        n_mat = len(mat)
        alpha = LETTERS[:n_mat]
        rng = chk.rng_for('edges asymmetric', name)
        pairs = []
        for n, m in ((80, 45), (geom['chunk'] + 37, 70)):
            ref = list(chk.random_seq(rng, n, alpha))
            ref[rng.randrange(n - 40)] = alpha[-1]                      # the highest code on both sides
            ref = ''.join(ref)
            a = max(0, n - 57 - m // 2) if n > geom['chunk'] else 10   # the copy straddles the chunk border
            qry = list(_copy(rng, ref, a, m, alpha, 0.15))
            qry[rng.randrange(m)] = alpha[-1]
            pairs.append((ref, ''.join(qry)))
        cases += _modes(pairs, mat, alpha, 5, 2)
    return cases


# ------------------------------------------------------------------------------------------------------------------------------
# row blocks: queries run in blocks of 64 rows; qv, vH, vE, outH, outE are exchanged by readlane / lane == rr, the store masked by `mine`
# ------------------------------------------------------------------------------------------------------------------------------
ROW_BLOCK_M = (63, 64, 65, 127, 128, 129)
ROW_BLOCK_SCORING = (2, 2, 3, 1)
PLANTED_INSERT = 75


def planted_insertion(geom):
    """(ref, query): 75 query letters the reference does not have on rows 51..125 (F over the border of row 64), and 25 reference
    letters the query does not have across the first chunk border (E over the hand-over), in one pair"""
    C = geom['chunk']
    rng = chk.rng_for('edges row blocks planted')
    ref = chk.random_seq(rng, C + 100, 'ACG')
    qry = ref[C - 100:C - 50] + 'T' * PLANTED_INSERT + ref[C - 50:C - 10] + ref[C + 15:C + 45]
    return ref, qry


def row_blocks(geom):
    cpl, C = geom['cpl'], geom['chunk']
    rng = chk.rng_for('edges row blocks')
    pairs = []
    for n in (cpl + 3, C, C + 1, 2 * C + cpl + 1):
        for m in ROW_BLOCK_M:
            ref = chk.random_seq(rng, n)
            border = C if n < 2 * C or m & 1 else 2 * C
            a = min(max(0, border - m // 2), max(0, n - m))
            pairs.append((ref, _copy(rng, ref, a, m, 'ACGT')))
    for m, n in ((64, C + 1), (129, cpl + 3), (65, 2 * C + cpl + 1)):
        pairs.append((chk.random_seq(rng, n), chk.random_seq(rng, m)))
    pairs.append(planted_insertion(geom))
    ma, mi, go, ge = ROW_BLOCK_SCORING
    return _modes(pairs, (ma, mi), None, go, ge)


# ------------------------------------------------------------------------------------------------------------------------------
# column geometry: L (lanes with a column in the last chunk), ln / kn (lane and register of column n), the nibble 4 * (p % cpl)
# ------------------------------------------------------------------------------------------------------------------------------
COLUMN_M = (1, 7, 70)


def column_lengths(geom):
    cpl, C = geom['cpl'], geom['chunk']
    single = [(5 + k) * cpl + k + 1 for k in range(cpl)]
    double = [C + (2 + k) * cpl + k + 1 for k in range(cpl)]
    return single + double + [C - cpl, C - 1, C + cpl - 1, C + cpl, C + cpl + 1, 2 * C, 3 * C - 1]


def planted_tail_deletion(rng, n, m, geom):
    """(ref, query): the query is ref[n - 2 cpl - m:n - 2 cpl] exactly, so the global alignment ends in a deletion of 2 cpl reference
    letters whose last one is column n: the walk starts inside a gap in the lane and register that own column n"""
    g = 2 * geom['cpl']
    ref = chk.random_seq(rng, n - g, 'ACG') + 'T' * g
    return ref, ref[n - g - m:n - g]


def column_geometry(geom):
    rng = chk.rng_for('edges column geometry')
    pairs = []
    for n in column_lengths(geom):
        for m in COLUMN_M:
            ref = chk.random_seq(rng, n)
            pairs.append((ref, _copy(rng, ref, max(0, n - m), m, 'ACGT')))            # a copy of the reference's end: the path reaches column n
            if m > 1 and n >= 2 * geom['cpl'] + m:
                pairs.append(planted_tail_deletion(rng, n, m, geom))
    return _modes(pairs, (2, 2), None, 3, 1)


# ------------------------------------------------------------------------------------------------------------------------------
# overlap ends: the last row before the last column, the last row's smallest column across chunks, the last column's smallest row
# across row blocks
# ------------------------------------------------------------------------------------------------------------------------------
LAST_COLUMN_M = 70
LAST_COLUMN_ROWS = (1, 63, 64, 65, LAST_COLUMN_M - 1)


def last_column_end(rng, n, i, m=LAST_COLUMN_M):
    """(ref, query) whose overlap alignment ends in the last column at row i with score min(i, n): the query is T beside the shared
    piece and the reference has no T, so no other cell of the last row or column reaches that score"""
    if n >= i:
        u = chk.random_seq(rng, i - 1, 'ACG') + 'G'
        return chk.random_seq(rng, n - i, 'AC') + u, u + 'T' * (m - i)
    u = chk.random_seq(rng, n - 1, 'ACG') + 'G'
    return u, 'T' * (i - n) + u + 'T' * (m - i)


def overlap_ends(geom):
    """-> [(name, Case)]; the names are what tests/test_ends_edges_host.py proves of each"""
    C = geom['chunk']
    rng = chk.rng_for('edges overlap ends')
    named = []
    for lu in (40, 41):
        for lx in (100, C - 63):            # n = 180, and s in chunk 0 with u in chunk 1
            s, u = chk.random_seq(rng, 40), chk.random_seq(rng, lu)
            x, y = chk.random_seq(rng, lx), chk.random_seq(rng, 60)
            named.append(('row ties column' if lu == 40 else 'column above row', (s + x + u, u + y + s)))
    for lu in (30, C + 5):
        u = chk.random_seq(rng, lu)
        a, b, c = chk.random_seq(rng, 10), chk.random_seq(rng, 100), chk.random_seq(rng, 15)
        named.append(('two in the last column', (u, a + u + b + u + c)))
    u = chk.random_seq(rng, 50)
    base = list(chk.random_seq(rng, 2 * C + 200))
    base[100:150] = u
    base[2 * C + 50:2 * C + 100] = u
    named.append(('two in the last row', (''.join(base), u)))
    for n in (5, C, C + 1, 2 * C + 3):
        for i in LAST_COLUMN_ROWS:
            named.append(('last column row %d' % i, last_column_end(rng, n, i)))
    named.append(('nothing in common', (chk.random_seq(rng, C + 40, 'AC'), chk.random_seq(rng, 70, 'GT'))))
    ma, mi, go, ge = OVERLAP_SCORING
    return [(name, Case(r, q, (ma, mi), None, go, ge, 'overlap')) for name, (r, q) in named]


# ------------------------------------------------------------------------------------------------------------------------------
# gap corners: with go == ge == 0 or go > ge == 0 almost every cell is a tie and the 4-bit decisions decide the whole CIGAR
# ------------------------------------------------------------------------------------------------------------------------------
def gap_corner_scorings():
    """-> [(scoring, alphabet, go, ge)]"""
    rng = chk.rng_for('edges gap corners matrices')
    pos = np.array([[rng.randint(1, 9) for _ in range(4)] for _ in range(4)], dtype=np.int64)
    neg = -np.array([[rng.randint(1, 9) for _ in range(4)] for _ in range(4)], dtype=np.int64)
    return [((2, 2), None, 0, 0), ((2, 2), None, 3, 0), ((1, 1), None, 7, 7), (pos, 'ACGT', 3, 1), (neg, 'ACGT', 3, 1)]


def gap_corners(geom):
    cpl, C = geom['cpl'], geom['chunk']
    cases = []
    for s, (scoring, alphabet, go, ge) in enumerate(gap_corner_scorings()):
        for alpha in ('AC', 'ACGT'):
            rng = chk.rng_for('edges gap corners', s, alpha)
            pairs = []
            for n in (cpl + 1, C + 9, 2 * C + 1):
                for m in (25, 70):
                    ref = chk.random_seq(rng, n, alpha)
                    a = max(0, min(n - m, C - m // 2))
                    pairs.append((ref, _copy(rng, ref, a, m, alpha) if (n + m) % 3 else chk.random_seq(rng, m, alpha)))
            cases += _modes(pairs, scoring, alphabet, go, ge)
    return cases


# ------------------------------------------------------------------------------------------------------------------------------
# int32 frame: the kernel adds (p + 1) ge - go, p up to chunk - 1, to a cell value; the host admits (m + n) max(|s|, go, ge) < 2^30
# ------------------------------------------------------------------------------------------------------------------------------
def frame_pairs(geom):
    C = geom['chunk']
    rng = chk.rng_for('edges int32 frame')
    ref = chk.random_seq(rng, C + 312)
    sq = chk.random_seq(rng, C)
    return [(ref, _copy(rng, ref, C - 100, 200, 'ACGT')), (sq, _copy(rng, sq, 0, C, 'ACGT'))]


def frame_limit(geom):
    """the largest gap cost the host admits for the first of frame_pairs: (m + n) * cost < 2^30"""
    return ((1 << 30) - 1) // (200 + geom['chunk'] + 312)


def int32_frame(geom):
    big = frame_limit(geom)
    pairs = frame_pairs(geom)
    return _modes(pairs, (2, 2), None, big, big) + _modes(pairs, (2, 2), None, big, 1)


# ------------------------------------------------------------------------------------------------------------------------------
# max runs: the host reserves min(m + n, 2 min(m, n) + 1) CIGAR ops for a pair
# ------------------------------------------------------------------------------------------------------------------------------
MAX_RUNS_SCORING = (5, 5, 1, 0)


def comb(rng, k):
    """(long, short): `short` is k letters A / C in turn, `long` holds them in order between k + 1 stretches of G / T, so the global
    alignment at 5 / 5 / 1 / 0 matches every short letter between k + 1 gaps: 2 k + 1 runs"""
    short = ''.join('AC'[t & 1] for t in range(k))
    gaps = [rng.choice('GT') * rng.randint(1, 3) for _ in range(k + 1)]
    return gaps[0] + ''.join(c + g for c, g in zip(short, gaps[1:])), short


def max_runs(geom):
    rng = chk.rng_for('edges max runs')
    pairs = [('TTAGGGCTT', 'AC')]
    for k in (5, 40):
        pairs.append(comb(rng, k))
    for k in (2, 5, 40):
        long_, short = comb(rng, k)
        pairs.append((short, long_))
    pairs.append(('A', 'C'))                       # 1I1D: min(m + n, 3) = 2 runs
    ma, mi, go, ge = MAX_RUNS_SCORING
    return _modes(pairs, (ma, mi), None, go, ge, modes=('global',))


def run_capacity(m, n):
    return min(m + n, 2 * min(m, n) + 1)


_max_runs_rows = {}


def max_runs_rows(geom):
    """-> (refs, queries, rows) of the max-runs pairs, rows[k] = (score, ref_begin, ref_end, query_begin, query_end, cigar text) as the
    one-piece checker states it (computed once).  Whatever plan aligns these pairs globally under costs that amount to
    MAX_RUNS_SCORING -- a second piece equal to the first, an intron too dear to open, a band that holds the whole matrix -- walks
    back through another instantiation of the walk and has to return the same rows, each with run_capacity(m, n) runs."""
    key = (geom['cpl'], geom['chunk'])
    if key not in _max_runs_rows:
        cases = max_runs(geom)
        wants = [expected(c) for c in cases]
        _max_runs_rows[key] = ([c.ref for c in cases], [c.query for c in cases], [chk.as_tuple(w)[:5] + (chk.cigar_text(w['cigar']),) for w in wants])
    return _max_runs_rows[key]


def check_max_runs(got, geom):
    """`got`: the PyAlignRes of the max-runs pairs from a plan as max_runs_rows describes"""
    refs, queries, rows = max_runs_rows(geom)
    assert len(got) == len(rows)
    for k, (g, r, q, row) in enumerate(zip(got, refs, queries, rows)):
        assert (g.score, g.ref_begin, g.ref_end, g.query_begin, g.query_end, g.cigar_string) == row, (k, r, q)
        assert len(chk.parse_cigar(g.cigar_string)) == run_capacity(len(q), len(r)), (k, r, q, g.cigar_string)


# ------------------------------------------------------------------------------------------------------------------------------
# shares: a plan cuts its batch so that the stored decisions of a share fit the workspace
# ------------------------------------------------------------------------------------------------------------------------------
SHARES_SCORING = (10, 4, 8, 2)
SHARES_MODES = ('semiglobal', 'global')
SHARES_WORKSPACES = ('default', 'max_pair_bytes', 'max_pair_bytes + 16')


def shares_pairs(geom):
    """9 (ref, query) of unequal size: two span several chunks with more than 64 rows, two have an empty side (the first pair, and the
    one directly after a large pair), the rest are small"""
    C = geom['chunk']
    rng = chk.rng_for('edges shares')
    shapes = [(0, 5), (20, 33), (100, C + 90), (7, 0), (5, 60), (33, 20), (70, 2 * C + 30), (64, 9), (12, 100)]      # (m, n)
    pairs = []
    for m, n in shapes:
        ref = chk.random_seq(rng, n)
        pairs.append((ref, _copy(rng, ref, max(0, min(n - m, C - m // 2)), m, 'ACGT')))
    assert [(len(q), len(r)) for r, q in pairs] == shapes
    return pairs


def pair_workspace_bytes(m, n, geom):
    """what the host reserves for the decisions of one pair: a word per row and lane with a column, rounded up to 16 bytes"""
    cpl, C = geom['cpl'], geom['chunk']
    nch = (n + C - 1) // C
    llast = (n - (nch - 1) * C + cpl - 1) // cpl
    return (4 * m * (64 * (nch - 1) + llast) + 15) & ~15


def share_count(shapes, workspace, geom):
    """the shares a plan with CIGARs cuts [(m, n)] into: a pair that no longer fits opens the next share; an empty side needs nothing"""
    count, used = 1, 0
    for m, n in shapes:
        if m and n:
            need = pair_workspace_bytes(m, n, geom)
            assert need <= workspace
            if used + need > workspace:
                count += 1; used = 0
            used += need
    return count


SETS = collections.OrderedDict([
    ('asymmetric', asymmetric), ('row blocks', row_blocks), ('column geometry', column_geometry),
    ('overlap ends', lambda geom: [c for _, c in overlap_ends(geom)]), ('gap corners', gap_corners), ('int32 frame', int32_frame),
    ('max runs', max_runs),
])
