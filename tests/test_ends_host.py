"""End-anchored affine-gap alignment (K1g) without a GPU: the checker (tests/ends_check.py) against the enumeration of every
alignment and against tests/edlib_check.py at unit costs, the kernel's scheme (tools/ends_model.py) against the checker at small
geometries, and the argument errors of ssw_wrap.align_pairs_ends."""
import itertools
import os
import sys

import numpy as np
import pytest

import edlib_check
import ends_check as chk

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
import ends_model as mdl  # noqa: E402

SCORINGS = [(10, 4, 8, 2), (2, 2, 3, 1), (1, 1, 1, 1), (1, 3, 2, 0)]


def _paths(m, n):
    """every alignment path of an m x n grid that starts on row 0 or column 0, as (start, end, diagonal cells as a bit mask, diagonals,
    gaps opened, gap letters beyond the first) -- walked step by step, no programme"""
    out = []

    def go(i, j, start, mask, nd, no, ne, last):
        out.append((start, (i, j), mask, nd, no, ne))
        if i < m and j < n:
            go(i + 1, j + 1, start, mask | (1 << (i * n + j)), nd + 1, no, ne, 'M')
        if i < m:
            go(i + 1, j, start, mask, nd, no + (last != 'I'), ne + (last == 'I'), 'I')
        if j < n:
            go(i, j + 1, start, mask, nd, no + (last != 'D'), ne + (last == 'D'), 'D')
    for j in range(n + 1):
        go(0, j, (0, j), 0, 0, 0, 0, None)
    for i in range(1, m + 1):
        go(i, 0, (i, 0), 0, 0, 0, 0, None)
    return out


def _allowed(mode, m, n, start, end):
    if mode == 'global':
        return start == (0, 0) and end == (m, n)
    if mode == 'semiglobal':
        return start[0] == 0 and end[0] == m
    return end[0] == m or end[1] == n


_POP = np.array([bin(x).count('1') for x in range(1 << 16)], dtype=np.int64)


@pytest.mark.parametrize('m', range(0, 5))
def test_checker_equals_the_best_of_every_enumerated_alignment(m):
    for n in range(0, 5):
        paths = _paths(m, n)
        per_mode = {}
        for mode in chk.MODES:
            sel = [p for p in paths if _allowed(mode, m, n, p[0], p[1])]
            per_mode[mode] = tuple(np.array([p[x] for p in sel], dtype=np.int64) for x in (2, 3, 4, 5))
        for qs in itertools.product('AC', repeat=m):
            for rs in itertools.product('AC', repeat=n):
                q, r = chk.encode(qs), chk.encode(rs)
                eq = sum(1 << (i * n + j) for i in range(m) for j in range(n) if qs[i] == rs[j])
                for mode in chk.MODES:
                    mask, nd, no, ne = per_mode[mode]
                    nm = _POP[mask & eq]
                    for ma, mi, go, ge in SCORINGS:
                        best = int((ma * nm - mi * (nd - nm) - go * no - ge * ne).max())
                        mat = chk.dna_matrix(ma, mi)
                        res = chk.plain(q, r, mat, go, ge, mode)
                        assert res['score'] == best, (qs, rs, mode, (ma, mi, go, ge), res, best)
                        chk.check_cigar(res, q, r, mat, go, ge, mode)
                        assert chk.as_tuple(chk.align(q, r, mat, go, ge, mode)) == chk.as_tuple(res)


def test_the_table_of_spans_without_a_letter():
    q, r, mat = chk.encode('AAAA'), chk.encode('CCCC'), chk.dna_matrix(10, 4)
    assert chk.as_tuple(chk.plain(q, r, mat, 8, 2, 'semiglobal')) == (-14, 0, -1, 0, 3, '4I')
    assert chk.as_tuple(chk.plain(q, r, mat, 8, 2, 'overlap')) == (0, 0, -1, 4, 3, '')
    assert chk.as_tuple(chk.plain(q, r, mat, 8, 2, 'global')) == (-16, 0, 3, 0, 3, '4M')


def test_row_form_equals_the_cell_form_on_longer_pairs():
    rng = chk.rng_for('rows vs cells')
    for t in range(60):
        alpha = 'AC' if t & 1 else 'ACGT'
        rs = chk.random_seq(rng, rng.randint(0, 90), alpha)
        qs = chk.mutate(rng, rs, 0.2, alpha) if t % 3 else chk.random_seq(rng, rng.randint(0, 90), alpha)
        ma, mi, go, ge = SCORINGS[t % 4]
        mat = chk.dna_matrix(ma, mi)
        for mode in chk.MODES:
            a = chk.plain(chk.encode(qs), chk.encode(rs), mat, go, ge, mode)
            b = chk.align(chk.encode(qs), chk.encode(rs), mat, go, ge, mode)
            assert chk.as_tuple(a) == chk.as_tuple(b), (qs, rs, mode)
            chk.check_cigar(b, chk.encode(qs), chk.encode(rs), mat, go, ge, mode)
            c = chk.align(chk.encode(qs), chk.encode(rs), mat, go, ge, mode, path=False)
            assert (c['score'], c['ref_end'], c['query_end']) == (a['score'], a['ref_end'], a['query_end'])


def test_unit_costs_give_the_edit_distances_of_the_edlib_checker():
    rng = chk.rng_for('edlib')
    mat = chk.dna_matrix(0, 1)
    eqm = edlib_check.eq_matrix()
    cases = [('ACGT', 'TTTT'), ('AAAA', 'CCCC'), ('A', 'A'), ('ACGTACGT', 'ACGT')]
    for t in range(150):
        alpha = 'AC' if t % 3 == 0 else 'ACGT'
        ts = chk.random_seq(rng, rng.randint(1, 60), alpha)
        qs = chk.mutate(rng, ts[rng.randint(0, len(ts) // 2):], 0.15, alpha) if t & 1 else chk.random_seq(rng, rng.randint(1, 25), alpha)
        if qs:
            cases.append((qs, ts))
    for qs, ts in cases:
        q, r = chk.encode(qs), chk.encode(ts)
        nw, _ = edlib_check.ends_of(edlib_check._arr(qs), edlib_check._arr(ts), 'NW', eqm)
        hw, ends = edlib_check.ends_of(edlib_check._arr(qs), edlib_check._arr(ts), 'HW', eqm)
        assert chk.align(q, r, mat, 1, 1, 'global')['score'] == -nw, (qs, ts)
        semi = chk.align(q, r, mat, 1, 1, 'semiglobal')
        assert semi['score'] == -hw and semi['ref_end'] == ends[0], (qs, ts, semi, hw, ends)
    assert any(edlib_check.ends_of(edlib_check._arr(a), edlib_check._arr(b), 'HW', eqm)[1][0] == -1 for a, b in cases)    # the seed column occurs


def _straddling(rng, C, alpha, kind):
    """a pair whose one long gap crosses the boundary between two chunks of C columns"""
    r = chk.random_seq(rng, 3 * C + rng.randint(0, 3), alpha)
    g = max(2, C // 2 + 1)
    at = rng.choice([C, 2 * C]) - g // 2
    if kind == 'deleted':
        return r[:at] + r[at + g:], r
    return r[:at] + chk.random_seq(rng, g, alpha) + r[at:], r


@pytest.mark.parametrize('lanes', [1, 2])
@pytest.mark.parametrize('cpl', [1, 2, 3, 7])
def test_model_equals_the_checker_at_small_geometries(cpl, lanes):
    rng = chk.rng_for('model', cpl, lanes)
    C = cpl * lanes
    pairs = []
    for t in range(40):
        alpha = 'AC' if t & 1 else 'ACGT'
        rs = chk.random_seq(rng, rng.choice([1, 2, C - 1, C, C + 1, 2 * C + 1, 3 * C + 2, rng.randint(1, 5 * C)]) or 1, alpha)
        qs = chk.mutate(rng, rs, 0.15, alpha) if t % 3 == 0 else chk.random_seq(rng, rng.randint(1, 3 * C + 3), alpha)
        pairs.append((qs or 'A', rs))
    for t in range(12):
        pairs.append(_straddling(rng, max(C, 4), 'AC' if t & 1 else 'ACGT', 'deleted' if t & 2 else 'added'))
    for t, (qs, rs) in enumerate(pairs):
        q, r = chk.encode(qs), chk.encode(rs)
        five = SCORINGS + [(2, 2, 3, 3)]
        for ma, mi, go, ge in (five[t % 5], five[(t + 2) % 5]):
            mat = chk.dna_matrix(ma, mi)
            for mode in chk.MODES:
                want = chk.align(q, r, mat, go, ge, mode)
                got = mdl.run(q, r, mat, go, ge, mode, cpl=cpl, lanes=lanes)
                assert chk.as_tuple(got) == chk.as_tuple(want), (t, qs, rs, mode, (ma, mi, go, ge))
                bare = mdl.run(q, r, mat, go, ge, mode, cpl=cpl, lanes=lanes, store=False)
                assert (bare['score'], bare['ref_end'], bare['query_end']) == (want['score'], want['ref_end'], want['query_end'])


def test_model_at_the_kernels_own_geometry_with_a_gap_across_the_hand_over():
    rng = chk.rng_for('model 8x64')
    r = chk.random_seq(rng, 1100, 'ACGT')
    q = r[:430] + r[600:]
    mat = chk.dna_matrix(2, 2)
    for mode in ('global', 'semiglobal'):
        want = chk.align(chk.encode(q[:60] + q[380:480]), chk.encode(r), mat, 3, 1, mode)
        got = mdl.run(chk.encode(q[:60] + q[380:480]), chk.encode(r), mat, 3, 1, mode, cpl=8, lanes=64)
        assert chk.as_tuple(got) == chk.as_tuple(want)


def test_argument_errors_are_raised_before_the_library_is_touched(monkeypatch):
    from ciri_long_amd import hip, ssw_wrap

    def boom(*a, **k):
        raise AssertionError('the library was touched')
    monkeypatch.setattr(hip, 'lib', boom)
    monkeypatch.setattr(hip, 'default_context', boom)
    with pytest.raises(ValueError, match='mode'):
        ssw_wrap.align_pairs_ends(['ACGT'], ['ACGT'], mode='local')
    with pytest.raises(ValueError, match='2 references vs 1 queries'):
        ssw_wrap.align_pairs_ends(['ACGT', 'AC'], ['ACGT'])
    with pytest.raises(ValueError, match='alphabet'):
        ssw_wrap.align_pairs_ends(['ARND'], ['ARND'], matrix=ssw_wrap.BLOSUM62)
    with pytest.raises(ValueError, match='alphabet'):
        ssw_wrap.align_pairs_ends(['ARND'], ['ARND'], alphabet=ssw_wrap.BLOSUM62_ALPHABET)
    with pytest.raises(ValueError, match='matrix'):
        ssw_wrap.align_pairs_ends(['ARND'], ['ARND'], matrix=ssw_wrap.BLOSUM62[:5, :5], alphabet=ssw_wrap.BLOSUM62_ALPHABET)
    assert ssw_wrap.align_pairs_ends([], []) == []
    with pytest.raises(ValueError, match='mode'):
        hip.EndsPlan(None, [], [0], [], [0], hip.score_matrix(2, 2), 3, 1, mode='nw')
