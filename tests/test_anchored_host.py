"""Start-anchored alignment of pairs (modes prefix, extend) without a GPU: the checker tests/anchored_check.py against the
enumeration of every alignment that starts at (0, 0), in the full matrix and under every admitted band; the Python models of K1g
and K1gb (tools/ends_model.py, tools/band_model.py) against the checker; prefix at unit costs against the edlib checker's SHW;
the band's certificate for a free end on seeded pairs; extend_anchors' stitching on a stand-in context; and planted faults in the
models, each caught by a named case set."""
import itertools
import os
import sys
import types

import numpy as np
import pytest

import anchored_check as chk
import edlib_check

TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools')
sys.path.insert(0, TOOLS)
import band_model as bmdl  # noqa: E402
import ends_model as emdl  # noqa: E402

SCORINGS = [(2, 2, 3, 1), (10, 4, 8, 2), (1, 1, 1, 1)]
FIVE = SCORINGS + [(1, 3, 2, 0), (2, 2, 3, 3)]            # ... plus ge = 0 and ge = go
SIX = FIVE + [(0, 1, 1, 1)]                               # ... plus unit costs


def _bands(mode, m, n):
    """every clipped band of an m x n pair that is not refused"""
    return [(lo, hi) for lo in range(-m, n + 1) for hi in range(lo, n + 1) if chk.refusal(mode, m, n, lo, hi) is None]


def _paths(m, n):
    """every alignment path of an m x n grid that starts at (0, 0), the empty one included, as (end, diagonal cells as a bit mask,
    diagonals, gaps opened, gap letters beyond the first, least and greatest diagonal j - i of its cells) -- walked step by step"""
    out = []

    def go(i, j, mask, nd, no, ne, last, dmin, dmax):
        dmin, dmax = min(dmin, j - i), max(dmax, j - i)
        out.append(((i, j), mask, nd, no, ne, dmin, dmax))
        if i < m and j < n:
            go(i + 1, j + 1, mask | (1 << (i * n + j)), nd + 1, no, ne, 'M', dmin, dmax)
        if i < m:
            go(i + 1, j, mask, nd, no + (last != 'I'), ne + (last == 'I'), 'I', dmin, dmax)
        if j < n:
            go(i, j + 1, mask, nd, no + (last != 'D'), ne + (last == 'D'), 'D', dmin, dmax)
    go(0, 0, 0, 0, 0, 0, None, 0, 0)
    return out


_POP = np.array([bin(x).count('1') for x in range(1 << 16)], dtype=np.int64)


@pytest.mark.parametrize('m', range(0, 5))
def test_checker_equals_the_best_of_every_enumerated_alignment_from_the_origin(m):
    t = 0
    for n in range(0, 5):
        paths = _paths(m, n)
        sel = {}
        for mode in chk.MODES:
            ps = [p for p in paths if mode == 'extend' or p[0][0] == m]
            for lo, hi in _bands(mode, m, n):
                inside = [p for p in ps if p[5] >= lo and p[6] <= hi]
                assert inside, (mode, m, n, lo, hi)                       # an admitted band holds an alignment
                ends = [p[0] for p in inside]
                sel[(mode, lo, hi)] = (ends,) + tuple(np.array([p[x] for p in inside], dtype=np.int64) for x in (1, 2, 3, 4))
        for qs in itertools.product('AC', repeat=m):
            for rs in itertools.product('AC', repeat=n):
                q, r = chk.encode(qs), chk.encode(rs)
                eq = sum(1 << (i * n + j) for i in range(m) for j in range(n) if qs[i] == rs[j])
                for (mode, lo, hi), (ends, mask, nd, no, ne) in sel.items():
                    nm = _POP[mask & eq]
                    t += 1
                    for ma, mi, go, ge in (FIVE[t % 5],) if (m + n) > 5 else FIVE:
                        scores = ma * nm - mi * (nd - nm) - go * no - ge * ne
                        best = int(scores.max())
                        end = min(ends[x] for x in np.flatnonzero(scores == best))         # smallest i, then smallest j
                        mat = chk.dna_matrix(ma, mi)
                        res = chk.plain_band(q, r, mat, go, ge, mode, lo, hi)
                        assert res['score'] == best and (res['query_end'] + 1, res['ref_end'] + 1) == end, \
                            (qs, rs, mode, (lo, hi), (ma, mi, go, ge), res, best, end)
                        chk.check_cigar(res, q, r, mat, go, ge, mode)
                        assert chk.as_tuple(chk.align_band(q, r, mat, go, ge, mode, lo, hi)) == chk.as_tuple(res), (qs, rs, mode, (lo, hi))
                        if (lo, hi) == (-m, n):                                            # the whole matrix: the unbanded programme
                            assert res['exact'] == 1
                            full = chk.plain(q, r, mat, go, ge, mode)
                            assert chk.as_tuple(full) == chk.as_tuple(res), (qs, rs, mode)
                            assert chk.as_tuple(chk.align(q, r, mat, go, ge, mode)) == chk.as_tuple(full), (qs, rs, mode)


def test_empty_sides_are_the_boundary():
    mat = chk.dna_matrix(2, 2)
    q, e = chk.encode('ACG'), chk.encode('')
    for f in (chk.plain, chk.align):
        assert chk.as_tuple(f(e, q, mat, 3, 1, 'extend')) == (0, 0, -1, 0, -1, '')
        assert chk.as_tuple(f(q, e, mat, 3, 1, 'extend')) == (0, 0, -1, 0, -1, '')
        assert chk.as_tuple(f(e, e, mat, 3, 1, 'prefix')) == (0, 0, -1, 0, -1, '')
        assert chk.as_tuple(f(e, q, mat, 3, 1, 'prefix')) == (0, 0, -1, 0, -1, '')
        assert chk.as_tuple(f(q, e, mat, 3, 1, 'prefix')) == (-5, 0, -1, 0, 2, '3I')


def test_row_forms_equal_the_cell_forms_on_longer_pairs():
    rng = chk.rng_for('anchored rows vs cells')
    seen = 0
    for t in range(200):
        alpha = 'AC' if t & 1 else 'ACGT'
        rs = chk.random_seq(rng, rng.randint(1, 60), alpha)
        qs = (chk.mutate(rng, rs[:rng.randint(1, 60)], 0.2, alpha) + chk.random_seq(rng, rng.randint(0, 20), alpha)) if t % 3 \
            else chk.random_seq(rng, rng.randint(1, 60), alpha)
        q, r = chk.encode(qs or 'A'), chk.encode(rs)
        m, n = len(q), len(r)
        ma, mi, go, ge = FIVE[t % 5]
        mat = chk.dna_matrix(ma, mi)
        for mode in chk.MODES:
            a = chk.plain(q, r, mat, go, ge, mode)
            assert chk.as_tuple(chk.align(q, r, mat, go, ge, mode)) == chk.as_tuple(a), (qs, rs, mode)
            chk.check_cigar(a, q, r, mat, go, ge, mode)
            c = chk.align(q, r, mat, go, ge, mode, path=False)
            assert (c['score'], c['ref_end'], c['query_end']) == (a['score'], a['ref_end'], a['query_end'])
            lo, hi = chk.band_of(m, n, rng.randint(0, 9), diag=rng.randint(-3, 3) if t % 4 == 0 else None)
            if chk.refusal(mode, m, n, lo, hi):
                continue
            seen += 1
            a = chk.plain_band(q, r, mat, go, ge, mode, lo, hi)
            b = chk.align_band(q, r, mat, go, ge, mode, lo, hi)
            assert chk.as_tuple(a) == chk.as_tuple(b) and (a['band'], a['exact']) == (b['band'], b['exact']), (qs, rs, mode, lo, hi)
            chk.check_cigar(b, q, r, mat, go, ge, mode)
            c = chk.align_band(q, r, mat, go, ge, mode, lo, hi, path=False)
            assert (c['score'], c['ref_end'], c['query_end'], c['exact']) == (a['score'], a['ref_end'], a['query_end'], a['exact'])
    assert seen > 250


def test_prefix_at_unit_costs_is_the_shw_of_the_edlib_checker():
    rng = chk.rng_for('anchored edlib')
    mat = chk.dna_matrix(0, 1)
    eqm = edlib_check.eq_matrix()
    cases = [('ACGT', 'TTTT'), ('AAAA', 'CCCC'), ('A', 'A'), ('ACGTACGT', 'ACGT'), ('ACGT', 'ACGTACGT')]
    for t in range(150):
        alpha = 'AC' if t % 3 == 0 else 'ACGT'
        ts = chk.random_seq(rng, rng.randint(1, 60), alpha)
        qs = chk.mutate(rng, ts[:rng.randint(1, len(ts))], 0.15, alpha) if t & 1 else chk.random_seq(rng, rng.randint(1, 25), alpha)
        if qs:
            cases.append((qs, ts))
    col0 = later = 0
    for qs, ts in cases:
        shw, ends = edlib_check.ends_of(edlib_check._arr(qs), edlib_check._arr(ts), 'SHW', eqm)
        got = chk.align(chk.encode(qs), chk.encode(ts), mat, 1, 1, 'prefix')
        # edlib's SHW never ends at column 0; the programme here does, where deleting the whole query (distance m) is as good
        want_end = -1 if shw == len(qs) else ends[0]
        assert got['score'] == -shw and got['ref_end'] == want_end, (qs, ts, got, shw, ends)
        col0 += shw == len(qs)
        later += ends[0] > 0 and shw < len(qs)
    assert col0 >= 2 and later > 50, (col0, later)


# ----------------------------------------------------------------------------------------------------------------------------
# the exact flag for a free end
# ----------------------------------------------------------------------------------------------------------------------------
def _exact_set(n_pairs=3000):
    """seeded pairs: lengths up to 40, alphabets AC and ACGT, six scorings, w from 0 to 12 -> (q, r, mat, go, ge, w); near-copies of
    a prefix with a diverged tail, and near-copies with one long gap, which pushes an alignment to the band's edge"""
    rng = chk.rng_for('anchored exact flag')
    for t in range(n_pairs):
        alpha = 'AC' if t & 1 else 'ACGT'
        rs = chk.random_seq(rng, rng.randint(1, 40), alpha)
        kind = t % 4
        if kind == 0:
            qs = chk.random_seq(rng, rng.randint(1, 40), alpha)
        elif kind == 1:
            qs = chk.mutate(rng, rs[:rng.randint(1, len(rs))], 0.15, alpha) + chk.random_seq(rng, rng.randint(0, 12), alpha)
        else:
            g, at = rng.randint(1, 14), rng.randint(0, len(rs))
            qs = (rs[:at] + rs[at + g:]) if kind == 2 else (rs[:at] + chk.random_seq(rng, g, alpha) + rs[at:])
            qs = chk.mutate(rng, qs, 0.05, alpha)
        ma, mi, go, ge = SIX[t % 6]
        yield chk.encode((qs or 'A')[:40]), chk.encode(rs), chk.dna_matrix(ma, mi), go, ge, rng.randint(0, 12)


def test_exact_flag_is_never_wrong_and_every_kind_of_pair_occurs():
    counts = {mode: dict(total=0, certified=0, equal_uncertified=0, unequal=0, refused=0) for mode in chk.MODES}
    pairs = 0
    for q, r, mat, go, ge, w in _exact_set():
        pairs += 1
        m, n = len(q), len(r)
        lo, hi = chk.band_of(m, n, w)
        for mode in chk.MODES:
            c = counts[mode]
            if chk.refusal(mode, m, n, lo, hi):
                c['refused'] += 1
                continue
            got = chk.align_band(q, r, mat, go, ge, mode, lo, hi)
            full = chk.align(q, r, mat, go, ge, mode)
            same = chk.as_tuple(got) == chk.as_tuple(full)
            c['total'] += 1
            if got['exact']:
                assert same, (mode, q, r, w, got, full)
                c['certified'] += 1
            else:
                assert (lo, hi) != (-m, n)
                c['equal_uncertified'] += same
                c['unequal'] += not same
    for mode in chk.MODES:
        print('exact flag, %s: %r' % (mode, counts[mode]))
    assert pairs >= 3000
    # the counts of this seeded set, checked on the CPU: every kind of pair occurs in both modes, and no certificate was wrong
    assert counts['extend'] == dict(total=3000, certified=1855, equal_uncertified=695, unequal=450, refused=0), counts['extend']
    assert counts['prefix'] == dict(total=2212, certified=1391, equal_uncertified=443, unequal=378, refused=788), counts['prefix']


def test_a_tie_with_the_bound_is_not_certified():
    # everything scores 0 and so does the bound of an alignment through diagonal hi + 1: the tie rules alone decide, no certificate
    mat = chk.dna_matrix(0, 0)
    for mode in chk.MODES:
        got = chk.align_band(chk.encode('AA'), chk.encode('AAAAA'), mat, 0, 0, mode, -2, 1)
        assert got['exact'] == 0 and got['score'] == 0
    assert chk.align_band(chk.encode('AA'), chk.encode('AAAAA'), chk.dna_matrix(2, 2), 3, 1, 'extend', -2, 1)['exact'] == 1     # 4 > 2 * 2 - 3 - 1


# ----------------------------------------------------------------------------------------------------------------------------
# the kernels' schemes
# ----------------------------------------------------------------------------------------------------------------------------
def _ends_agree(model, case):
    qs, rs, mat, go, ge, mode, cpl, lanes = case
    q, r = chk.encode(qs), chk.encode(rs)
    want = chk.align(q, r, mat, go, ge, mode)
    try:
        got = model.run(q, r, mat, go, ge, mode, cpl=cpl, lanes=lanes)
        bare = model.run(q, r, mat, go, ge, mode, cpl=cpl, lanes=lanes, store=False)
    except (AssertionError, KeyError, IndexError):
        return False
    return chk.as_tuple(got) == chk.as_tuple(want) and \
        (bare['score'], bare['ref_end'], bare['query_end']) == (want['score'], want['ref_end'], want['query_end'])


def _ends_cases(name, cpl, lanes):
    """the named case sets of the K1g model, at the geometry cpl x lanes (a chunk is C = cpl * lanes columns)"""
    rng = chk.rng_for('anchored ends model', name, cpl, lanes)
    C = cpl * lanes
    out = []
    if name == 'random':
        for t in range(40):
            alpha = 'AC' if t & 1 else 'ACGT'
            rs = chk.random_seq(rng, rng.choice([1, 2, C - 1, C, C + 1, 2 * C + 1, 3 * C + 2, rng.randint(1, 5 * C)]) or 1, alpha)
            qs = (chk.mutate(rng, rs[:rng.randint(1, len(rs))], 0.15, alpha) + chk.random_seq(rng, rng.randint(0, C + 2), alpha)) if t % 3 == 0 \
                else chk.random_seq(rng, rng.randint(1, 3 * C + 3), alpha)
            five = SCORINGS + [(2, 2, 3, 3), (1, 3, 2, 0)]
            for ma, mi, go, ge in (five[t % 5], five[(t + 2) % 5]):
                for mode in chk.MODES:
                    out.append((qs or 'A', rs, chk.dna_matrix(ma, mi), go, ge, mode, cpl, lanes))
    elif name == 'zero scores':                    # every cell ties with (0, 0): the empty result, whatever the lane meets later
        for m, n in ((1, 1), (2, C + 1), (3, 2 * C + 2)):
            for mode in chk.MODES:
                out.append(('A' * m, 'A' * n, chk.dna_matrix(0, 0), 0, 0, mode, cpl, lanes))
    elif name == 'all mismatch':                   # nothing scores above 0: extend gives the empty result
        for m, n in ((1, 1), (3, C + 2), (C + 1, 2)):
            for mode in chk.MODES:
                out.append(('A' * m, 'C' * n, chk.dna_matrix(2, 2), 3, 1, mode, cpl, lanes))
    elif name == 'ties across chunks':
        # free gaps, match 1, mismatch 0: H is the length of a common subsequence.  'CA' against 'A' G.. 'C' (the C in chunk 2): the
        # best, 1, is at (1, C + 1) in chunk 2 and at (2, 1) in chunk 1, which the lane-private search meets first.  'AC' against 'A'
        # G.. is the reverse: 1 at (1, 1) in chunk 1 and again all along row 1 in chunk 2
        free = chk.dna_matrix(1, 0)
        for extra in (0, 1, C):
            out.append(('CA', 'A' + 'G' * (C - 1) + 'C' + 'G' * extra, free, 0, 0, 'extend', cpl, lanes))
            out.append(('AC', 'A' + 'G' * (C + extra), free, 0, 0, 'extend', cpl, lanes))
            out.append(('GCA', 'A' + 'T' * (2 * C - 1) + 'C' + 'T' * extra, free, 0, 0, 'extend', cpl, lanes))
    return out


ENDS_SETS = ('random', 'zero scores', 'all mismatch', 'ties across chunks')


@pytest.mark.parametrize('lanes', [1, 2])
@pytest.mark.parametrize('cpl', [1, 2, 3, 7])
def test_ends_model_equals_the_checker_at_small_geometries(cpl, lanes):
    n = 0
    for name in ENDS_SETS:
        for case in _ends_cases(name, cpl, lanes):
            assert _ends_agree(emdl, case), (name, case[:2], case[3:])
            n += 1
    assert n > 150


def test_ends_model_at_the_kernels_own_geometry():
    rng = chk.rng_for('anchored model 8x64')
    r = chk.random_seq(rng, 1100, 'ACGT')
    q = chk.mutate(rng, r[:40], 0.1) + chk.random_seq(rng, 30)
    for mode in chk.MODES:
        assert _ends_agree(emdl, (q, r, chk.dna_matrix(2, 2), 3, 1, mode, 8, 64))
    for case in _ends_cases('ties across chunks', 8, 64)[:2]:
        assert _ends_agree(emdl, case)


def _band_agree(model, case):
    """case: ..., w, diag: the band is the model's own (band_of), as the host gives it"""
    qs, rs, mat, go, ge, mode, w, diag, cpl, lanes = case
    q, r = chk.encode(qs), chk.encode(rs)
    m, n = len(q), len(r)
    lo, hi = chk.band_of(m, n, w, diag)
    want = chk.align_band(q, r, mat, go, ge, mode, lo, hi)
    try:
        mlo, mhi = model.band_of(mode, m, n, w, diag)
        got = model.run(q, r, mat, go, ge, mode, mlo, mhi, cpl=cpl, lanes=lanes)
        bare = model.run(q, r, mat, go, ge, mode, mlo, mhi, cpl=cpl, lanes=lanes, store=False)
    except (AssertionError, KeyError, IndexError):
        return False
    return chk.as_tuple(got) + (got['band'], got['exact']) == chk.as_tuple(want) + (want['band'], want['exact']) and \
        (bare['score'], bare['ref_end'], bare['query_end'], bare['exact']) == (want['score'], want['ref_end'], want['query_end'], want['exact'])


def _band_cases(name, cpl, lanes):
    rng = chk.rng_for('anchored band model', name, cpl, lanes)
    W = cpl * lanes
    big = W > 64
    out = []

    def add(qs, rs, mat, go, ge, mode, w, diag=None):
        m, n = len(qs), len(rs)
        ulo, uhi = chk.band_unclipped(w, diag)
        lo, hi = chk.band_of(m, n, w, diag)
        if chk.refusal(mode, m, n, ulo, uhi) is None and hi - lo + 1 <= W:
            out.append((qs, rs, mat, go, ge, mode, w, diag, cpl, lanes))
    if name == 'random':
        for t in range(10 if big else 60):
            alpha = 'AC' if t & 1 else 'ACGT'
            n = rng.randint(1, 24 if big else 3 * W + 6)
            rs = chk.random_seq(rng, n, alpha)
            qs = (chk.mutate(rng, rs[:rng.randint(1, n)], 0.15, alpha) + chk.random_seq(rng, rng.randint(0, 8), alpha)) if t % 3 \
                else chk.random_seq(rng, rng.randint(1, 24 if big else 3 * W + 6), alpha)
            ma, mi, go, ge = FIVE[t % 5]
            for mode in chk.MODES:
                if t & 2:
                    add(qs or 'A', rs, chk.dna_matrix(ma, mi), go, ge, mode, rng.randint(0, W // 2), diag=rng.randint(-2, 2))
                else:
                    add(qs or 'A', rs, chk.dna_matrix(ma, mi), go, ge, mode, rng.randint(0, (W - 1) // 2))
    elif name == 'unequal lengths':                # m and n far apart under a default band: n - m plays no part
        for t in range(2 if big else 8):
            rs = chk.random_seq(rng, rng.randint(12, 20) if big else 2 * W + 8 + t, 'ACGT')
            qs = chk.mutate(rng, rs[:len(rs) // 3], 0.1)
            for mode in chk.MODES:
                add(qs or 'A', rs, chk.dna_matrix(2, 2), 3, 1, mode, 1 if big else max(0, (W - 1) // 2))
                add(rs, qs or 'A', chk.dna_matrix(2, 2), 3, 1, 'extend', 1 if big else max(0, (W - 1) // 2))
    elif name == 'exact ties':                     # the banded score EQUALS the bound of an alignment through diagonal hi + 1
        for k in (1, 2):
            for mode in chk.MODES:
                add('A' * k, 'A' * (k + 3), chk.dna_matrix(0, 0), 0, 0, mode, 1)
    elif name == 'zero scores and all mismatch':
        for m, n in ((1, 1), (3, 5), (6, 2)):
            add('A' * m, 'A' * n, chk.dna_matrix(0, 0), 0, 0, 'extend', 2)
            add('A' * m, 'C' * n, chk.dna_matrix(2, 2), 3, 1, 'extend', 2)
    return out


BAND_SETS = ('random', 'unequal lengths', 'exact ties', 'zero scores and all mismatch')


@pytest.mark.parametrize('lanes', [1, 2, 64])
@pytest.mark.parametrize('cpl', [1, 2, 3, 8])
def test_band_model_equals_the_checker(cpl, lanes):
    n = 0
    for name in BAND_SETS:
        for case in _band_cases(name, cpl, lanes):
            assert _band_agree(bmdl, case), (name, case[:2], case[3:])
            n += 1
    assert n >= 8, n


def _mutant(module, old, new):
    path = os.path.join(TOOLS, module + '.py')
    with open(path) as f:
        src = f.read()
    assert src.count(old) == 1, (old, src.count(old))
    ns = {'__name__': module + '_mutant'}
    exec(compile(src.replace(old, new), path, 'exec'), ns)
    return types.SimpleNamespace(run=ns['run'], band_of=ns.get('band_of'))


MUTANTS = [
    ('>= for > in the best-cell update', 'ends_model', 'chunk_best[l] is None or H[l][k] > chunk_best[l][0]',
     'chunk_best[l] is None or H[l][k] >= chunk_best[l][0]', ('random',)),
    ('the cross-chunk tie by value only', 'ends_model', 'if cv > ext[l][0] or (cv == ext[l][0] and ci < ext[l][1]):', 'if cv > ext[l][0]:',
     ('ties across chunks',)),
    ('(0, 0) not seeded', 'ends_model', 'ext = [(0, 0, 0)] * lanes', 'ext = [(-(1 << 40), 0, 0)] * lanes', ('all mismatch', 'zero scores')),
    ('>= for > in the band\'s best-cell update', 'band_model', 'if H[p] > ext[p // cpl][0]:', 'if H[p] >= ext[p // cpl][0]:',
     ('zero scores and all mismatch',)),
    ('(0, 0) not seeded in the band', 'band_model', 'ext = [(0, 0, 0)] * lanes', 'ext = [(-(1 << 29), 0, 0)] * lanes', ('zero scores and all mismatch',)),
    ('>= in the exact rule', 'band_model', 'free = free and score > splus * min(m, n - hi - 1)', 'free = free and score >= splus * min(m, n - hi - 1)',
     ('exact ties',)),
    ('the default band taken from n - m', 'band_model', "elif mode in ('prefix', 'extend'):\n        lo, hi = -w, w", 'elif False:\n        lo, hi = -w, w',
     ('unequal lengths',)),
]


@pytest.mark.parametrize('name,module,old,new,sets', MUTANTS, ids=[m[0] for m in MUTANTS])
def test_a_planted_fault_in_a_model_is_caught_by_a_named_set(name, module, old, new, sets):
    model = _mutant(module, old, new)
    good, agree, cases_of = (emdl, _ends_agree, _ends_cases) if module == 'ends_model' else (bmdl, _band_agree, _band_cases)
    caught = []
    for s in sets:
        cases = cases_of(s, 2, 2) + cases_of(s, 3, 1)
        assert cases and all(agree(good, c) for c in cases), s                 # the model as it stands passes the set
        if any(not agree(model, c) for c in cases):
            caught.append(s)
    print('%s: caught by %s' % (name, ', '.join(caught)))
    assert caught == list(sets), (name, caught)


# ----------------------------------------------------------------------------------------------------------------------------
# the wrapper
# ----------------------------------------------------------------------------------------------------------------------------
class _StandIn(object):
    """a context whose ends_batch and band_batch are the checker: what extend_anchors sends and how it stitches, without a device"""

    def __init__(self):
        self.calls = []

    def _rows(self, dtype, qd, qo, rd, ro, mat, go, ge, mode, want_cigar, band=None, diagonals=None):
        edge = int(round(len(mat) ** 0.5))
        mat = np.asarray(mat, dtype=np.int64).reshape(edge, edge)
        rows = np.zeros(len(qo) - 1, dtype=dtype)
        cig = []
        self.calls.append((mode, len(rows), band))
        for k in range(len(rows)):
            q, r = np.asarray(qd[qo[k]:qo[k + 1]], dtype=np.int64), np.asarray(rd[ro[k]:ro[k + 1]], dtype=np.int64)
            if band is None:
                res = chk.align(q, r, mat, go, ge, mode)
            else:
                lo, hi = chk.band_of(len(q), len(r), band, None if diagonals is None else diagonals[k])
                res = chk.align_band(q, r, mat, go, ge, mode, lo, hi)
                rows[k]['band_lo'], rows[k]['band_hi'], rows[k]['exact'] = lo, hi, res['exact']
            for f in ('score', 'ref_begin', 'ref_end', 'query_begin', 'query_end'):
                rows[k][f] = res[f]
            rows[k]['cigar_off'], rows[k]['cigar_len'] = (len(cig), len(res['cigar'])) if want_cigar else (-1, 0)
            if want_cigar:
                cig += [(n << 4) | 'MID'.index(o) for o, n in res['cigar']]
        return rows, np.array(cig, dtype=np.uint32)

    def ends_batch(self, qd, qo, rd, ro, mat, go, ge, mode='global', want_cigar=True, workspace_bytes=0):
        from ciri_long_amd import hip
        return self._rows(hip.ENDS_DTYPE, qd, qo, rd, ro, mat, go, ge, mode, want_cigar)

    def band_batch(self, qd, qo, rd, ro, mat, go, ge, band, mode='global', diagonals=None, want_cigar=True, workspace_bytes=0):
        from ciri_long_amd import hip
        return self._rows(hip.BAND_DTYPE, qd, qo, rd, ro, mat, go, ge, mode, want_cigar, band, diagonals)


@pytest.mark.parametrize('band', [None, 6])
def test_extend_anchors_stitches_two_extend_halves(band):
    from ciri_long_amd import ssw_wrap
    rng = chk.rng_for('stitch', band)
    scoring = (2, 2, 3, 1)
    for seed_len in (0, 7):
        reads = chk.anchored_reads(rng, 30, seed_len=seed_len, lo=8, hi=40)
        reads.append(('ACGT', 'ACGT', (0, 0)) if seed_len == 0 else ('ACGTACGT', 'ACGTACG', (0, 0)))
        reads.append(('ACGT', 'TTTT', (4 - seed_len, 4 - seed_len)) if seed_len == 0 else ('GGACGTACG', 'ACGTACG', (2, 0)))
        ctx = _StandIn()
        got = ssw_wrap.extend_anchors([x[0] for x in reads], [x[1] for x in reads], [x[2] for x in reads], band=band, seed_len=seed_len,
                                      match=2, mismatch=2, gap_open=3, gap_extend=1, report_cigar=True, context=ctx)
        assert ctx.calls == [('extend', 2 * len(reads), band)]                 # both halves of all pairs in one plan
        for (rs, qs, anchor), g in zip(reads, got):
            want, exact = chk.expected_anchor(rs, qs, anchor, seed_len, scoring, band)
            assert (g.score, g.ref_begin, g.ref_end, g.query_begin, g.query_end, g.cigar_string) == want[:5] + (chk.text_of(want, len(qs)),), (rs, qs, anchor)
            assert (g.band_exact == exact) if band is not None else not hasattr(g, 'band_exact')
            # the stitched CIGAR is one alignment of the span it states, and costs the score
            ops = [(o, n) for o, n in chk.parse_cigar(g.cigar_string) if o != 'S']
            score, nr, nq = chk.rescore(ops, chk.encode(qs), chk.encode(rs), g.ref_begin, g.query_begin, chk.dna_matrix(2, 2), 3, 1)
            assert (score, g.ref_begin + nr - 1, g.query_begin + nq - 1) == (g.score, g.ref_end, g.query_end)
            assert all(a[0] != b[0] for a, b in zip(ops, ops[1:]))
        bare = ssw_wrap.extend_anchors([x[0] for x in reads], [x[1] for x in reads], [x[2] for x in reads], band=band, seed_len=seed_len,
                                       match=2, mismatch=2, gap_open=3, gap_extend=1, context=_StandIn())
        assert [(b.score, b.ref_begin, b.ref_end, b.query_begin, b.query_end, b.cigar_string) for b in bare] == \
            [(g.score, g.ref_begin, g.ref_end, g.query_begin, g.query_end, None) for g in got]


def test_argument_errors_are_raised_before_the_library_is_touched(monkeypatch):
    from ciri_long_amd import hip, ssw_wrap

    def boom(*a, **k):
        raise AssertionError('the library was touched')
    monkeypatch.setattr(hip, 'lib', boom)
    monkeypatch.setattr(hip, 'default_context', boom)
    assert hip.ENDS_MODES['prefix'] == 3 and hip.ENDS_MODES['extend'] == 4
    with pytest.raises(ValueError, match='mode'):
        ssw_wrap.align_pairs_ends(['ACGT'], ['ACGT'], mode='suffix')
    with pytest.raises(ValueError, match='not built'):
        ssw_wrap.align_pairs_band(['ACGT'], ['ACGT'], 2, mode='overlap')
    with pytest.raises(ValueError, match='1 references vs 1 queries vs 0 anchors'):
        ssw_wrap.extend_anchors(['ACGT'], ['ACGT'], [])
    with pytest.raises(ValueError, match=r'pair 0: the anchor \(3, 0\) with seed_len 2 lies outside the 4 x 4 pair'):
        ssw_wrap.extend_anchors(['ACGT'], ['ACGT'], [(3, 0)], seed_len=2)
    with pytest.raises(ValueError, match='half-width'):
        ssw_wrap.extend_anchors(['ACGT'], ['ACGT'], [(0, 0)], band=-1)
    with pytest.raises(ValueError, match='seed_len'):
        ssw_wrap.extend_anchors(['ACGT'], ['ACGT'], [(0, 0)], seed_len=-1)
    assert ssw_wrap.extend_anchors([], [], []) == []
