"""Banded end-anchored alignment (K1gb) without a GPU: the checker (tests/band_check.py) against the enumeration of every alignment
inside the band and, with the band wide open, against tests/ends_check.py; the exact flag against the unbanded programme; the
kernel's scheme (tools/band_model.py) against the checker at small and at the real geometries; one-line faults planted in the model,
each caught by a named case set; and the argument errors of ssw_wrap.align_pairs_band."""
import itertools
import os
import sys

import numpy as np
import pytest

import band_check as chk
import ends_check as ec

TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools')
sys.path.insert(0, TOOLS)
import band_model as mdl  # noqa: E402

SCORINGS = [(2, 2, 3, 1), (10, 4, 8, 2), (1, 1, 1, 1)]
FIVE = SCORINGS + [(1, 3, 2, 0), (2, 2, 3, 3)]            # ... plus ge = 0 and ge = go
SIX = FIVE + [(0, 1, 1, 1)]                               # ... plus unit costs


def _bands(mode, m, n):
    """every clipped band of an m x n pair that is not refused"""
    return [(lo, hi) for lo in range(-m, n + 1) for hi in range(lo, n + 1) if chk.refusal(mode, m, n, lo, hi) is None]


def _paths(m, n):
    """every alignment path of an m x n grid that starts on row 0, as (start, end, diagonal cells as a bit mask, diagonals, gaps
    opened, gap letters beyond the first, least and greatest diagonal j - i of its cells) -- walked step by step, no programme"""
    out = []

    def go(i, j, start, mask, nd, no, ne, last, dmin, dmax):
        dmin, dmax = min(dmin, j - i), max(dmax, j - i)
        out.append((start, (i, j), mask, nd, no, ne, dmin, dmax))
        if i < m and j < n:
            go(i + 1, j + 1, start, mask | (1 << (i * n + j)), nd + 1, no, ne, 'M', dmin, dmax)
        if i < m:
            go(i + 1, j, start, mask, nd, no + (last != 'I'), ne + (last == 'I'), 'I', dmin, dmax)
        if j < n:
            go(i, j + 1, start, mask, nd, no + (last != 'D'), ne + (last == 'D'), 'D', dmin, dmax)
    for j in range(n + 1):
        go(0, j, (0, j), 0, 0, 0, 0, None, j, j)
    return out


_POP = np.array([bin(x).count('1') for x in range(1 << 16)], dtype=np.int64)


@pytest.mark.parametrize('m', range(0, 5))
def test_checker_equals_the_best_of_every_enumerated_alignment_inside_the_band(m):
    t = 0
    for n in range(0, 5):
        paths = _paths(m, n)
        sel = {}
        for mode in chk.MODES:
            ps = [p for p in paths if p[1][0] == m and (p[0] == (0, 0) and p[1] == (m, n) if mode == 'global' else True)]
            for lo, hi in _bands(mode, m, n):
                inside = [p for p in ps if p[6] >= lo and p[7] <= hi]
                assert inside, (mode, m, n, lo, hi)                       # an admitted band holds an alignment
                sel[(mode, lo, hi)] = tuple(np.array([p[x] for p in inside], dtype=np.int64) for x in (2, 3, 4, 5))
        for qs in itertools.product('AC', repeat=m):
            for rs in itertools.product('AC', repeat=n):
                q, r = chk.encode(qs), chk.encode(rs)
                eq = sum(1 << (i * n + j) for i in range(m) for j in range(n) if qs[i] == rs[j])
                for (mode, lo, hi), (mask, nd, no, ne) in sel.items():
                    nm = _POP[mask & eq]
                    t += 1
                    for ma, mi, go, ge in (FIVE[t % 5], FIVE[(t + 2) % 5]) if (m + n) > 5 else FIVE:
                        best = int((ma * nm - mi * (nd - nm) - go * no - ge * ne).max())
                        mat = chk.dna_matrix(ma, mi)
                        res = chk.plain(q, r, mat, go, ge, mode, lo, hi)
                        assert res['score'] == best, (qs, rs, mode, (lo, hi), (ma, mi, go, ge), res, best)
                        chk.check_cigar(res, q, r, mat, go, ge, mode)
                        assert chk.as_tuple(chk.align(q, r, mat, go, ge, mode, lo, hi)) == chk.as_tuple(res), (qs, rs, mode, (lo, hi))


def _length_grid(rng):
    pairs = []
    for n in (0, 1, 2, 7, 31, 64, 90):
        for m in (0, 1, 2, 5, 33, 70):
            alpha = 'AC' if (m + n) & 1 else 'ACGT'
            rs = chk.random_seq(rng, n, alpha)
            pairs.append((chk.random_seq(rng, m, alpha), rs))
            pairs.append(((chk.mutate(rng, rs, 0.15, alpha) + chk.random_seq(rng, m, alpha))[:m], rs))
    return pairs


def test_with_the_band_wide_open_the_checker_equals_the_unbanded_one_field_by_field():
    rng = chk.rng_for('band wide open')
    for t, (qs, rs) in enumerate(_length_grid(rng)):
        q, r = chk.encode(qs), chk.encode(rs)
        m, n = len(q), len(r)
        for ma, mi, go, ge in FIVE:
            mat = chk.dna_matrix(ma, mi)
            for mode in chk.MODES:
                want = ec.as_tuple(ec.align(q, r, mat, go, ge, mode))
                for w in (m + n, 10 ** 6):
                    lo, hi = chk.band_of(m, n, w)
                    assert (lo, hi) == (-m, n)
                    got = chk.align(q, r, mat, go, ge, mode, lo, hi)
                    assert ec.as_tuple(got) == want and got['exact'] == 1, (qs, rs, mode, (ma, mi, go, ge))
                if m * n <= 700:
                    assert chk.as_tuple(chk.plain(q, r, mat, go, ge, mode, -m, n)) == chk.as_tuple(got)
                    assert ec.as_tuple(ec.plain(q, r, mat, go, ge, mode)) == want


def test_row_form_equals_the_cell_form_and_every_cigar_rescores_and_stays_inside_the_band():
    rng = chk.rng_for('band rows vs cells')
    seen = 0
    for t in range(240):
        alpha = 'AC' if t & 1 else 'ACGT'
        rs = chk.random_seq(rng, rng.randint(1, 60), alpha)
        qs = chk.mutate(rng, rs, 0.2, alpha) if t % 3 else chk.random_seq(rng, rng.randint(1, 60), alpha)
        q, r = chk.encode(qs), chk.encode(rs)
        m, n = len(q), len(r)
        ma, mi, go, ge = FIVE[t % 5]
        mat = chk.dna_matrix(ma, mi)
        for mode in chk.MODES:
            if t % 4 == 0:
                lo, hi = chk.band_of(m, n, rng.randint(0, 9), diag=rng.randint(-m, n))
            else:
                lo, hi = chk.band_of(m, n, rng.randint(0, 9))
            if chk.refusal(mode, m, n, lo, hi):
                continue
            seen += 1
            a = chk.plain(q, r, mat, go, ge, mode, lo, hi)
            b = chk.align(q, r, mat, go, ge, mode, lo, hi)
            assert chk.as_tuple(a) == chk.as_tuple(b), (qs, rs, mode, lo, hi)
            chk.check_cigar(b, q, r, mat, go, ge, mode)
            c = chk.align(q, r, mat, go, ge, mode, lo, hi, path=False)
            assert (c['score'], c['ref_end'], c['query_end'], c['exact']) == (a['score'], a['ref_end'], a['query_end'], a['exact'])
    assert seen > 300


# ----------------------------------------------------------------------------------------------------------------------------
# the exact flag
# ----------------------------------------------------------------------------------------------------------------------------
def _exact_set(n_pairs=3000):
    """seeded random pairs: lengths up to 40, alphabets AC and ACGT, six scorings, w from 0 to 12 -> (q, r, mat, go, ge, w)"""
    rng = chk.rng_for('exact flag')
    for t in range(n_pairs):
        alpha = 'AC' if t & 1 else 'ACGT'
        rs = chk.random_seq(rng, rng.randint(1, 40), alpha)
        kind = t % 4
        if kind == 0:
            qs = chk.random_seq(rng, rng.randint(1, 40), alpha)
        elif kind == 1:
            qs = chk.mutate(rng, rs, 0.15, alpha) or 'A'
        else:                                                   # a near-copy with one long gap: what pushes an alignment to the band's edge
            g, at = rng.randint(1, 14), rng.randint(0, len(rs))
            qs = (rs[:at] + rs[at + g:]) if kind == 2 else (rs[:at] + chk.random_seq(rng, g, alpha) + rs[at:])
            qs = chk.mutate(rng, qs, 0.05, alpha) or 'A'
        ma, mi, go, ge = SIX[t % 6]
        yield chk.encode(qs[:40]), chk.encode(rs), chk.dna_matrix(ma, mi), go, ge, rng.randint(0, 12)


def test_exact_flag_is_never_wrong_and_both_kinds_of_uncertified_pairs_occur():
    certified = equal = unequal_uncertified = equal_uncertified = total = 0
    for q, r, mat, go, ge, w in _exact_set():
        m, n = len(q), len(r)
        lo, hi = chk.band_of(m, n, w)
        got = chk.align(q, r, mat, go, ge, 'global', lo, hi)
        full = ec.plain(q, r, mat, go, ge, 'global')
        same = ec.as_tuple(got) == ec.as_tuple(full)
        total += 1
        certified += got['exact']
        equal += same
        if got['exact']:
            assert same, (q, r, w, got, full)
        else:
            assert (lo, hi) != (-m, n)
            equal_uncertified += same
            unequal_uncertified += not same
    print('exact flag: %d pairs, %d certified, %d equal, %d equal without certificate, %d unequal'
          % (total, certified, equal, equal_uncertified, unequal_uncertified))
    assert total >= 3000 and certified > total // 3 and equal_uncertified > 20 and unequal_uncertified > 20


def test_semiglobal_rows_are_certified_only_when_the_band_is_the_whole_matrix():
    rng = chk.rng_for('exact semiglobal')
    mat = chk.dna_matrix(10, 4)
    r = chk.encode(chk.random_seq(rng, 30))
    q = r[10:20]
    for w, want in ((5, 0), (9, 0), (10, 1)):
        lo, hi = chk.band_of(len(q), len(r), w)
        assert chk.align(q, r, mat, 8, 2, 'semiglobal', lo, hi)['exact'] == want, (w, lo, hi)
    # an alignment can lie outside a semiglobal band without ever crossing it: the better copy is simply elsewhere
    r2 = np.concatenate([q[:9], [(q[9] + 1) % 4], r[:8], q])
    inside = chk.align(q, r2, mat, 8, 2, 'semiglobal', *chk.band_of(len(q), len(r2), 2, diag=0))
    full = ec.align(q, r2, mat, 8, 2, 'semiglobal')
    assert inside['exact'] == 0 and inside['score'] < full['score'] and full['ref_begin'] == 18


def zigzag():
    """a 300-letter reference; the query is the same with 30 letters removed at 80 and 30 random letters added at 200"""
    rng = chk.rng_for('zigzag')
    ref = chk.random_seq(rng, 300)
    cut = ref[:80] + ref[110:]
    qry = cut[:170] + chk.random_seq(rng, 30) + cut[170:]      # position 200 of the reference
    assert len(qry) == 300
    return qry, ref


def test_the_zigzag_pair_loses_at_29_and_is_exact_at_30():
    qs, rs = zigzag()
    q, r, mat = chk.encode(qs), chk.encode(rs), chk.dna_matrix(10, 4)
    full = ec.align(q, r, mat, 8, 2, 'global')
    narrow = chk.align(q, r, mat, 8, 2, 'global', *chk.band_of(300, 300, 29))
    wide = chk.align(q, r, mat, 8, 2, 'global', *chk.band_of(300, 300, 30))
    print('zigzag: w = 29 scores %d, w = 30 scores %d, the full matrix %d (%s)' % (narrow['score'], wide['score'], full['score'], ec.cigar_text(full['cigar'])))
    assert narrow['score'] < full['score'] and narrow['exact'] == 0
    assert ec.as_tuple(wide) == ec.as_tuple(full) and wide['exact'] == 1
    assert '30D' in ec.cigar_text(full['cigar']) and '30I' in ec.cigar_text(full['cigar'])
    chk.check_cigar(narrow, q, r, mat, 8, 2, 'global')
    chk.check_cigar(wide, q, r, mat, 8, 2, 'global')


# ----------------------------------------------------------------------------------------------------------------------------
# the kernel's scheme
# ----------------------------------------------------------------------------------------------------------------------------
def _agree(model, case):
    qs, rs, scoring, mode, lo, hi, cpl, lanes = case
    ma, mi, go, ge = scoring
    q, r, mat = chk.encode(qs), chk.encode(rs), chk.dna_matrix(ma, mi)
    want = chk.align(q, r, mat, go, ge, mode, lo, hi)
    try:
        got = model.run(q, r, mat, go, ge, mode, lo, hi, cpl=cpl, lanes=lanes)
        bare = model.run(q, r, mat, go, ge, mode, lo, hi, cpl=cpl, lanes=lanes, store=False)
    except (AssertionError, KeyError, IndexError):
        return False
    return chk.as_tuple(got) == chk.as_tuple(want) and \
        (bare['score'], bare['ref_end'], bare['query_end'], bare['exact']) == (want['score'], want['ref_end'], want['query_end'], want['exact'])


def _cases(name, cpl, lanes):
    """the named case sets of the model tests, at the geometry cpl x lanes"""
    rng = chk.rng_for('band model', name, cpl, lanes)
    W = cpl * lanes
    big = W > 64                                   # the model costs W positions a row: few, short pairs at the real geometries
    out = []
    if name == 'random':                           # random and near-copy pairs under default bands and hints of every width that fits
        for t in range(10 if big else 60):
            alpha = 'AC' if t & 1 else 'ACGT'
            n = rng.randint(1, 24 if big else 3 * W + 6)
            rs = chk.random_seq(rng, n, alpha)
            qs = (chk.mutate(rng, rs, 0.15, alpha) if t % 3 else chk.random_seq(rng, rng.randint(1, 24 if big else 3 * W + 6), alpha)) or 'A'
            m = len(qs)
            for mode in chk.MODES:
                if t & 2:
                    lo, hi = chk.band_of(m, n, rng.randint(0, W), diag=rng.randint(-m, n))
                else:
                    lo, hi = chk.band_of(m, n, rng.randint(0, W))
                if hi - lo + 1 <= W and chk.refusal(mode, m, n, lo, hi) is None:
                    out.append((qs, rs, FIVE[t % 5], mode, lo, hi, cpl, lanes))
    elif name == 'gaps at the edge':               # one gap of exactly the half-width each way: the path touches hi, then lo
        w = 9 if big else max(1, (W - 1) // 2)
        for t in range(2 if big else 6):
            rs = chk.random_seq(rng, 4 * w + 12 + t, 'ACGT')
            cut = rs[:w + 3] + rs[2 * w + 3:]
            qs = cut[:2 * w + 6] + chk.random_seq(rng, w, 'ACGT') + cut[2 * w + 6:]
            for scoring in ((10, 4, 8, 2), (10, 4, 8, 0), (10, 4, 8, 8)):
                for ww in (w, w - 1):
                    lo, hi = chk.band_of(len(qs), len(rs), ww)
                    out.append((qs, rs, scoring, 'global', lo, hi, cpl, lanes))
    elif name == 'column 0 and column n':          # bands that hold column 0 for some rows only, and run off column n
        for t in range(3 if big else 12):
            n = rng.randint(2, 10 if big else W + 4)
            m = rng.randint(2, 10 if big else W + 4)
            rs, qs = chk.random_seq(rng, n, 'AC'), chk.random_seq(rng, m, 'AC')
            for mode in chk.MODES:
                for lo, hi in ((max(-m, -2), min(n, W - 3)), (max(-m, -1), min(n, 1)), (-min(m, W - 1), 0)):
                    if 0 < hi - lo + 1 <= W and chk.refusal(mode, m, n, lo, hi) is None:
                        out.append((qs, rs, FIVE[t % 5], mode, lo, hi, cpl, lanes))
    elif name == 'long rows':                      # more rows than positions: every letter of the window has slid through
        for t in range(1 if big else 4):
            rs = chk.random_seq(rng, 70 if big else 4 * W + 9, 'ACGT')
            qs = chk.mutate(rng, rs, 0.1, 'ACGT')
            for mode in chk.MODES:
                lo, hi = chk.band_of(len(qs), len(rs), 3 if big else max(0, (W - abs(len(qs) - len(rs)) - 1) // 2))
                out.append((qs, rs, SCORINGS[t % 3], mode, lo, hi, cpl, lanes))
    return out


SETS = ('random', 'gaps at the edge', 'column 0 and column n', 'long rows')


@pytest.mark.parametrize('lanes', [1, 2, 64])
@pytest.mark.parametrize('cpl', [1, 2, 3, 8])
def test_model_equals_the_checker(cpl, lanes):
    n = 0
    for name in SETS:
        for case in _cases(name, cpl, lanes):
            if case[5] - case[4] + 1 > cpl * lanes:
                continue
            assert _agree(mdl, case), (name, case)
            n += 1
    assert n >= 8, n


def _mutant(old, new):
    path = os.path.join(TOOLS, 'band_model.py')
    with open(path) as f:
        src = f.read()
    assert src.count(old) == 1, (old, src.count(old))
    ns = {'__name__': 'band_model_mutant'}
    exec(compile(src.replace(old, new), path, 'exec'), ns)

    class _M(object):
        run = staticmethod(ns['run'])
    return _M


MUTANTS = [
    ('F taken from b instead of b + 1', 'F[p] = _any(max(hu - go, fu - ge))', 'F[p] = _any(max(Hp[p] - go, Fp[p] - ge))', ('random', 'gaps at the edge')),
    ('the letter window does not slide', 'rc = rc[1:] + [letter(lo + W + i)]', 'rc = rc', ('random', 'long rows')),
    ('the entering letter is one column off', 'rc = rc[1:] + [letter(lo + W + i)]', 'rc = rc[1:] + [letter(lo + W + i - 1)]', ('long rows',)),
    ('the position left of column 0 stays a cell one row too long', 'ok = [0 <= jr[p] <= n', 'ok = [-1 <= jr[p] <= n', ('column 0 and column n',)),
    ('the position right of column n is a cell', 'ok = [0 <= jr[p] <= n', 'ok = [0 <= jr[p] <= n + 1', ('column 0 and column n', 'random')),
    ('the upper band edge left open', 'jr = [lo + p + 1 if p < B else', 'jr = [lo + p + 1 if p < B + 1 else', ('gaps at the edge',)),
    ('E seeded with a score instead of minus infinity', 'u = incl[l - 1] if l else NEG', 'u = incl[l - 1] if l else 0', ('random',)),
    ('>= in the exact rule', 'ok = ok and score > splus * max(0, n - hi - 1)', 'ok = ok and score >= splus * max(0, n - hi - 1)', ('exact ties',)),
]


def _exact_ties(cpl, lanes):
    """pairs whose banded score EQUALS the bound of an alignment through diagonal hi + 1, under a band open below: 'A' x k against 'A' x
    (k + 3) scored 0 / 0 / 0 / 0 -- every alignment scores 0, so does the bound, and the tie rules alone decide the CIGAR: no certificate"""
    return [('A' * k, 'A' * (k + 3), (0, 0, 0, 0), 'global', -k, 3, cpl, lanes) for k in (1, 2)]


@pytest.mark.parametrize('name,old,new,sets', MUTANTS, ids=[m[0] for m in MUTANTS])
def test_a_planted_fault_in_the_model_is_caught_by_a_named_set(name, old, new, sets):
    model = _mutant(old, new)
    caught = []
    for s in sets:
        cases = _exact_ties(3, 2) if s == 'exact ties' else _cases(s, 2, 2) + _cases(s, 3, 1)
        assert all(_agree(mdl, c) for c in cases), s                 # the model as it stands passes the set
        if any(not _agree(model, c) for c in cases):
            caught.append(s)
    print('%s: caught by %s' % (name, ', '.join(caught)))
    assert caught == list(sets), (name, caught)


def test_admission_bound_of_the_model_keeps_minus_infinity_apart():
    # the largest gap cost the bound admits for a 6 x 7 pair: every value the model meets passes its range checks (_score, _any)
    m, n = 6, 7
    go = ((1 << 29) - 1) // (m + n + 2 * mdl.MAX_WIDTH)
    assert mdl.admitted(m, n, go) and not mdl.admitted(m, n, go + 1)
    rng = chk.rng_for('bound')
    q, r = chk.encode(chk.random_seq(rng, m)), chk.encode(chk.random_seq(rng, n))
    mat = chk.dna_matrix(127, 127)
    for ge in (0, go):
        for mode in chk.MODES:
            lo, hi = chk.band_of(m, n, 2)
            got = mdl.run(q, r, mat, go, ge, mode, lo, hi, cpl=8, lanes=64)
            assert chk.as_tuple(got) == chk.as_tuple(chk.align(q, r, mat, go, ge, mode, lo, hi))


def test_argument_errors_are_raised_before_the_library_is_touched(monkeypatch):
    from ciri_long_amd import hip, ssw_wrap

    def boom(*a, **k):
        raise AssertionError('the library was touched')
    monkeypatch.setattr(hip, 'lib', boom)
    monkeypatch.setattr(hip, 'default_context', boom)
    with pytest.raises(ValueError, match='not built'):
        ssw_wrap.align_pairs_band(['ACGT'], ['ACGT'], 4, mode='overlap')
    with pytest.raises(ValueError, match='mode'):
        ssw_wrap.align_pairs_band(['ACGT'], ['ACGT'], 4, mode='local')
    with pytest.raises(ValueError, match='2 references vs 1 queries'):
        ssw_wrap.align_pairs_band(['ACGT', 'AC'], ['ACGT'], 4)
    with pytest.raises(ValueError, match='1 diagonals vs 2 pairs'):
        ssw_wrap.align_pairs_band(['ACGT', 'AC'], ['ACGT', 'AC'], 4, diagonals=[0])
    with pytest.raises(ValueError, match='half-width'):
        ssw_wrap.align_pairs_band(['ACGT'], ['ACGT'], -1)
    with pytest.raises(ValueError, match='alphabet'):
        ssw_wrap.align_pairs_band(['ARND'], ['ARND'], 4, matrix=ssw_wrap.BLOSUM62)
    assert ssw_wrap.align_pairs_band([], [], 4) == []
    assert hip.BAND_DTYPE.itemsize == 48 and hip.BAND_DTYPE.fields['band_lo'][1] == 32
