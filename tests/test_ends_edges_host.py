"""CPU statements to tests/ends_edges.py: the two forms of the checker (tests/ends_check.py) against each other on the edge sets, the
kernel's scheme (tools/ends_model.py) at the real geometry (8 columns per lane, 64 lanes, decisions stored) against the checker, the
proof that every set reaches what it is named for, and the proof that the sets have teeth: seven one-line faults planted in the model's
source are each caught by a named set.

The model is pure Python at about 2 us a cell, padding included, so it runs on the cheapest case of each distinct shape of a set (mode,
scoring, chunks, row blocks, for the column set the register that owns column n, for the overlap set every construction) within
MODEL_CELLS cells per set, cheapest first; the checker runs on every case."""
import os
import sys

import numpy as np
import pytest

import ends_check as chk
import ends_edges as E

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
import ends_model as mdl  # noqa: E402

GEOM = E.HOST_GEOM
CPL, CHUNK = GEOM['cpl'], GEOM['chunk']
MODEL_CELLS = 800000

_cases, _want = {}, {}


def cases_of(name):
    if name not in _cases:
        _cases[name] = E.SETS[name](GEOM)
        assert _cases[name], name
    return _cases[name]


def want_of(case):
    """the checker's answer, computed once and shared"""
    key = (case.ref, case.query, E.scoring_key(case))
    if key not in _want:
        _want[key] = E.expected(case)
    return _want[key]


def _padded_cells(case):
    return len(case.query) * ((len(case.ref) + CHUNK - 1) // CHUNK) * CHUNK


def _planted(name):
    """the (ref, query) the model always runs: what a set plants on purpose"""
    if name == 'row blocks':
        return {E.planted_insertion(GEOM)}
    if name == 'overlap ends':
        return {(c.ref, c.query) for what, c in E.overlap_ends(GEOM) if not what.startswith('last column row') and len(c.query) <= 200}
    return set()


def model_subset(name):
    """every case where the whole set fits MODEL_CELLS; else what the set plants on purpose, then the cheapest case of each distinct
    shape, cheapest shapes first, while they fit"""
    cases = cases_of(name)
    if sum(_padded_cells(c) for c in cases) <= MODEL_CELLS:
        return list(cases)
    best = {}
    planted = _planted(name)
    for c in cases:
        m, n = len(c.query), len(c.ref)
        shape = (E.scoring_key(c), (n + CHUNK - 1) // CHUNK, (m + 63) // 64, (n - 1) % CPL if name == 'column geometry' else 0)
        if name == 'overlap ends':              # every construction is a shape of its own
            shape = (c.ref, c.query)
        if shape not in best or _padded_cells(c) < _padded_cells(best[shape]):
            best[shape] = c
    out = [c for c in cases if (c.ref, c.query) in planted]
    total = sum(_padded_cells(c) for c in out)
    for c in sorted((c for c in best.values() if (c.ref, c.query) not in planted), key=_padded_cells):
        if total + _padded_cells(c) > MODEL_CELLS:
            break
        out.append(c); total += _padded_cells(c)
    assert out, name
    return out


def _model(case, model=mdl, **kw):
    q, r = E.codes_of(case)
    return model.run(q, r, E.matrix_of(case), case.go, case.ge, case.mode, cpl=CPL, lanes=CHUNK // CPL, store=True, **kw)


@pytest.mark.parametrize('name', list(E.SETS))
def test_both_forms_of_the_checker_on_every_case(name):
    small = 0
    for c in cases_of(name):
        q, r = E.codes_of(c)
        want = want_of(c)
        chk.check_cigar(want, q, r, E.matrix_of(c), c.go, c.ge, c.mode)
        bare = E.expected(c, path=False)
        assert (bare['score'], bare['ref_end'], bare['query_end']) == (want['score'], want['ref_end'], want['query_end'])
        if len(q) * len(r) <= 4000:
            small += 1
            assert chk.as_tuple(chk.plain(q, r, E.matrix_of(c), c.go, c.ge, c.mode)) == chk.as_tuple(want), c
    assert small or name == 'int32 frame'
    assert all(len(c.query) <= 200 and len(c.ref) <= 3 * CHUNK + CPL for c in cases_of(name)
               if not (name == 'overlap ends' and len(c.ref) == CHUNK + 5) and not (name == 'int32 frame' and len(c.query) == CHUNK))


@pytest.mark.parametrize('name', [n for n in E.SETS if n != 'int32 frame'])
def test_model_at_the_real_geometry(name):
    for c in model_subset(name):
        assert chk.as_tuple(_model(c)) == chk.as_tuple(want_of(c)), c


# ----------------------------------------------------------------------------------------------------------------------------
# the sets prove their own edges
# ----------------------------------------------------------------------------------------------------------------------------
def test_asymmetric_a_transposed_matrix_changes_the_answer_for_every_matrix_in_every_mode():
    cases = cases_of('asymmetric')
    names = E.asymmetric_matrices()
    assert [len(m) for _, m in names] == [2, 5, 20, 32, 5] and names[-1][1].min() == -128 and names[-1][1].max() == 127
    assert all(-9 <= m.min() and m.max() <= 9 for _, m in names[:-1])
    changed = set()
    for c in cases:
        n_mat = len(c.scoring)
        q, r = E.codes_of(c)
        assert q.max() == n_mat - 1 == r.max()
        assert len(c.ref) in (80, CHUNK + 37)
        flipped = chk.align(q, r, E.matrix_of(c).T, c.go, c.ge, c.mode)
        if chk.as_tuple(flipped) != chk.as_tuple(want_of(c)):
            changed.add((c.scoring.tobytes(), c.mode))
    assert changed == {(m.tobytes(), mode) for _, m in names for mode in E.MODES}


def _runs_with_rows(want, op):
    """[(length, first query row, last query row)] of the runs of `op`, rows 1-based"""
    i, out = want['query_begin'], []
    for o, k in want['cigar']:
        if o == op:
            out.append((k, i + 1, i + k))
        if o != 'D':
            i += k
    return out


def test_row_blocks_the_lengths_and_the_planted_insertion_across_row_64():
    cases = cases_of('row blocks')
    want_n = {CPL + 3, CHUNK, CHUNK + 1, 2 * CHUNK + CPL + 1}
    for mode in E.MODES:
        assert {(len(c.query), len(c.ref)) for c in cases if c.mode == mode} >= {(m, n) for m in E.ROW_BLOCK_M for n in want_n}
    planted = [c for c in cases if (c.ref, c.query) == E.planted_insertion(GEOM)]
    assert [c.mode for c in planted] == list(E.MODES)
    for c in planted:
        w = want_of(c)
        long_ = [x for x in _runs_with_rows(w, 'I') if x[0] >= 70]
        assert len(long_) == 1 and long_[0][1] <= 64 and long_[0][2] >= 65, (c.mode, w['cigar'])
        # and a deletion over the first chunk border in the same pair: E crosses the hand-over
        j, over = w['ref_begin'], []
        for o, k in w['cigar']:
            if o == 'D' and j < CHUNK < j + k:
                over.append(k)
            if o != 'I':
                j += k
        assert over and over[0] >= 20, (c.mode, w['cigar'])


def test_column_geometry_every_register_owns_column_n_in_one_chunk_and_in_the_last_of_two():
    cases = cases_of('column geometry')
    for mode in E.MODES:
        for m in E.COLUMN_M:
            ns = {len(c.ref) for c in cases if c.mode == mode and len(c.query) == m}
            assert {(n - 1) % CPL for n in ns if n <= CHUNK - CPL} == set(range(CPL))
            assert {(n - 1) % CPL for n in ns if CHUNK < n < 2 * CHUNK} == set(range(CPL))
            assert ns >= {CHUNK - CPL, CHUNK - 1, CHUNK + CPL - 1, CHUNK + CPL, CHUNK + CPL + 1, 2 * CHUNK, 3 * CHUNK - 1}
            assert len({(n + CPL - 1) // CPL for n in ns if n <= CHUNK}) >= CPL          # L varies as well
    # the planted deletion: the global walk starts in a gap of 2 cpl letters at column n, for every register
    ends_in_gap = set()
    for c in cases:
        if c.mode == 'global' and c.ref.endswith('T' * (2 * CPL)) and want_of(c)['cigar'][-1] == ('D', 2 * CPL):
            ends_in_gap.add((len(c.ref) - 1) % CPL)
    assert ends_in_gap == set(range(CPL))


def test_overlap_ends_the_ties_are_ties():
    named = E.overlap_ends(GEOM)
    seen = set()
    for name, c in named:
        q, r = E.codes_of(c)
        m, n = len(q), len(r)
        w = want_of(c)
        row, col = chk.last_row_and_column(q, r, E.matrix_of(c), c.go, c.ge, c.mode)
        assert len(row) == n + 1 and len(col) == m + 1
        top_row, top_col = max(row), max(col[:m])
        seen.add(name)
        if name == 'row ties column':
            assert top_row == top_col == 40 and (w['score'], w['ref_end'], w['query_end']) == (40, 39, m - 1)
            assert row.count(40) == 1 and col[:m].count(40) == 1
        elif name == 'column above row':
            assert (top_row, top_col) == (40, 41) and (w['score'], w['ref_end'], w['query_end']) == (41, n - 1, 40)
        elif name == 'two in the last column':
            ties = [i for i in range(m) if col[i] == top_col]
            assert top_col == n > top_row and len(ties) == 2 and w['query_end'] == ties[0] - 1 and w['ref_end'] == n - 1
            assert (ties[0] - 1) // 64 != (ties[1] - 1) // 64
            if n == 30:
                assert ((ties[0] - 1) // 64, (ties[1] - 1) // 64) == (0, 2)
        elif name == 'two in the last row':
            ties = [j for j in range(n + 1) if row[j] == top_row]
            assert top_row == m > top_col and len(ties) == 2 and w['ref_end'] == ties[0] - 1 and w['query_end'] == m - 1
            assert ((ties[0] - 1) // CHUNK, (ties[1] - 1) // CHUNK) == (0, 2)
        elif name.startswith('last column row '):
            i = int(name.split()[-1])
            assert top_col == min(i, n) > top_row and col[:m].count(top_col) == 1
            assert (w['score'], w['ref_end'], w['query_end']) == (min(i, n), n - 1, i - 1)
            seen.add((i, n))
        else:
            assert name == 'nothing in common'
            assert chk.as_tuple(w) == (0, 0, -1, m, m - 1, '') and top_col == 0
    assert seen >= {'row ties column', 'column above row', 'two in the last column', 'two in the last row', 'nothing in common'}
    assert seen >= {(i, n) for i in E.LAST_COLUMN_ROWS for n in (5, CHUNK, CHUNK + 1, 2 * CHUNK + 3)}
    assert {len(c.ref) for name, c in named if name == 'two in the last column'} == {30, CHUNK + 5}


def test_gap_corners_the_scorings_and_the_ties():
    cases = cases_of('gap corners')
    sc = E.gap_corner_scorings()
    assert [(s if a is None else None, go, ge) for s, a, go, ge in sc] == [((2, 2), 0, 0), ((2, 2), 3, 0), ((1, 1), 7, 7), (None, 3, 1), (None, 3, 1)]
    assert sc[3][0].min() > 0 and sc[4][0].max() < 0 and sc[3][0].shape == sc[4][0].shape == (4, 4)
    for mode in E.MODES:
        shapes = {(len(c.query), len(c.ref), ''.join(sorted(set(c.ref)))) for c in cases if c.mode == mode and c.go == 0}
        assert shapes == {(m, n, a) for m in (25, 70) for n in (CPL + 1, CHUNK + 9, 2 * CHUNK + 1) for a in ('AC', 'ACGT')}
    # with free gaps a path is many ties long: more runs than a scored gap would ever pay for
    free = [want_of(c) for c in cases if c.go == 0 and c.mode == 'global' and len(c.ref) > CHUNK]
    assert free and all(len(w['cigar']) > 20 for w in free)


def test_int32_frame_the_model_reaches_two_to_the_29_and_stays_inside_int32():
    cases = cases_of('int32 frame')
    big = E.frame_limit(GEOM)
    assert big == (1 << 20) - 1
    assert {(len(c.query), len(c.ref)) for c in cases} == {(200, CHUNK + 312), (CHUNK, CHUNK)}
    assert {(c.go, c.ge, c.mode) for c in cases} == {(big, ge, mode) for ge in (big, 1) for mode in E.MODES}
    for c in cases:
        m, n = len(c.query), len(c.ref)
        assert (m + n) * big < 1 << 30 <= (m + n) * (big + 1)
    unequal = [want_of(c)['score'] for c in cases if c.mode == 'global' and c.ge == big and len(c.query) == 200]
    assert len(unequal) == 1 and -7.0e8 < unequal[0] < -6.0e8
    # the model on the unequal pair in every mode with go == ge, on the global one with ge == 1 too, and on the square pair once
    ran = 0
    for c in cases:
        if (len(c.query) == 200 and (c.ge == big or c.mode == 'global')) or (c.mode, c.ge) == ('semiglobal', big):
            peak = []
            got = _model(c, extreme=peak)                 # _i32 inside: no value the kernel forms leaves int32
            assert chk.as_tuple(got) == chk.as_tuple(want_of(c)), (c.mode, c.go, c.ge)
            assert len(peak) == 1 and peak[0] < 1 << 31
            if c.mode == 'global' and c.ge == big:
                assert peak[0] >= 1 << 29, (c.mode, peak)
            ran += 1
    assert ran == 5


def test_max_runs_every_cigar_fills_what_the_host_reserves():
    cases = cases_of('max runs')
    assert all(c.mode == 'global' for c in cases)
    assert chk.cigar_text(want_of(cases[0])['cigar']) == '2D1M3D1M2D'
    shapes = set()
    for c in cases:
        m, n = len(c.query), len(c.ref)
        w = want_of(c)
        assert len(w['cigar']) == E.run_capacity(m, n) == min(m + n, 2 * min(m, n) + 1), (m, n, w['cigar'])
        shapes.add((min(m, n), 'D' if n > m else ('I' if m > n else '=')))
    assert shapes >= {(2, 'D'), (5, 'D'), (40, 'D'), (2, 'I'), (5, 'I'), (40, 'I'), (1, '=')}


def test_shares_the_pairs_and_the_cuts_they_imply():
    pairs = E.shares_pairs(GEOM)
    shapes = [(len(q), len(r)) for r, q in pairs]
    assert len(pairs) == 9 and len(set(shapes)) == 9
    large = [k for k, (m, n) in enumerate(shapes) if n > CHUNK and m > 64]
    empty = [k for k, (m, n) in enumerate(shapes) if not m or not n]
    assert len(large) == 2 and empty == [0, large[0] + 1]
    need = [E.pair_workspace_bytes(m, n, GEOM) if m and n else 0 for m, n in shapes]
    top = max(need)
    assert sorted(need)[-2] * 2 > top > 8 * sorted(need)[-3]           # the two large pairs never share; the small ones are far below them
    for order in (shapes, shapes[::-1]):
        assert E.share_count(order, 1 << 30, GEOM) == 1
        assert E.share_count(order, top, GEOM) >= 3 and E.share_count(order, top + 16, GEOM) >= 2
    assert E.pair_workspace_bytes(100, CHUNK + 90, GEOM) == 4 * 100 * (64 + 12) and E.pair_workspace_bytes(1, 1, GEOM) == 16
    ma, mi, go, ge = E.SHARES_SCORING
    ran = 0
    for r, q in pairs:
        if q and r and len(q) * len(r) <= 20000:
            for mode in E.SHARES_MODES:
                c = E.Case(r, q, (ma, mi), None, go, ge, mode)
                assert chk.as_tuple(_model(c)) == chk.as_tuple(want_of(c))
                ran += 1
    assert ran == 10


# ----------------------------------------------------------------------------------------------------------------------------
# the sets have teeth
# ----------------------------------------------------------------------------------------------------------------------------
# (name, line of tools/ends_model.py, what replaces it, the sets asked in turn)
MUTANTS = [
    ('matrix lookup transposed', 'int(mat[r[j - 1]][q[i - 1]]) if j <= n else 0', 'int(mat[q[i - 1]][r[j - 1]]) if j <= n else 0',
     ('asymmetric', 'gap corners')),
    ('last row no longer before the last column', "or row_best >= col_best:", "or row_best > col_best:", ('overlap ends', 'gap corners')),
    ('last column takes its largest row', 'hn > col_best:', 'hn >= col_best:', ('overlap ends',)),
    ('last row takes its largest column', 'if h > row_best:', 'if h >= row_best:', ('overlap ends', 'column geometry', 'gap corners')),
    ('F before E as the source of H', '(1 if H[l][k] == E[l][k] else 2)', '(2 if H[l][k] == F[l][k] else 1)', ('gap corners', 'max runs')),
    ('handed-over E ignored', 'hin, ein = hand[(c - 1) & 1][i - 1]\n', 'hin, ein = hand[(c - 1) & 1][i - 1]; ein = hin - go\n',
     ('row blocks', 'gap corners')),
    ('E opened here judged with ge', 'E[l][k] == left - go', 'E[l][k] == left - ge', ('max runs', 'row blocks')),
]


def _mutant(old, new):
    path = os.path.join(os.path.dirname(os.path.abspath(mdl.__file__)), 'ends_model.py')
    with open(path) as f:
        src = f.read()
    assert src.count(old) == 1, (old, src.count(old))
    ns = {'__name__': 'ends_model_mutant'}
    exec(compile(src.replace(old, new), path, 'exec'), ns)

    class _M(object):
        run = staticmethod(ns['run'])
    return _M


def _disagrees(model, case):
    try:
        return chk.as_tuple(_model(case, model=model)) != chk.as_tuple(want_of(case))
    except (AssertionError, KeyError, IndexError):             # a walk that leaves the stored words is a disagreement too
        return True


@pytest.mark.parametrize('name,old,new,sets', MUTANTS, ids=[m[0] for m in MUTANTS])
def test_a_planted_fault_in_the_model_is_caught_by_a_named_set(name, old, new, sets):
    model = _mutant(old, new)
    caught = [s for s in sets if any(_disagrees(model, c) for c in sorted(model_subset(s), key=_padded_cells))]
    print('%s: caught by %s' % (name, ', '.join(caught)))
    assert caught == list(sets), (name, caught)


def test_the_unchanged_source_passes_where_the_mutants_fail():
    model = _mutant('def run(', 'def run(')
    for s in ('max runs', 'overlap ends'):
        assert not any(_disagrees(model, c) for c in model_subset(s)[:6])


# ----------------------------------------------------------------------------------------------------------------------------
# a matrix entry outside int8 is refused, not wrapped
# ----------------------------------------------------------------------------------------------------------------------------
def test_a_matrix_entry_outside_int8_raises_and_names_the_entry(monkeypatch):
    from ciri_long_amd import hip, ssw_wrap

    def boom(*a, **k):
        raise AssertionError('the library was touched')
    monkeypatch.setattr(hip, 'lib', boom)
    monkeypatch.setattr(hip, 'default_context', boom)
    for bad, where in ((128, (1, 2)), (-129, (3, 0)), (300, (3, 3))):
        mat = np.arange(16, dtype=np.int64).reshape(4, 4)
        mat[where] = bad
        with pytest.raises(ValueError, match=r'matrix\[%d\]\[%d\] = %d is outside -128\.\.127' % (where + (bad,))):
            ssw_wrap.align_pairs_ends(['ACGT'], ['ACGT'], matrix=mat, alphabet='ACGT')
        with pytest.raises(ValueError, match=r'matrix\[%d\]\[%d\] = %d is outside -128\.\.127' % (where + (bad,))):
            ssw_wrap.align_pairs_matrix(['ACGT'], ['ACGT'], mat, 'ACGT', 3, 1)
        with pytest.raises(ValueError, match=r'matrix\[%d\] = %d is outside -128\.\.127' % (where[0] * 4 + where[1], bad)):
            ssw_wrap.align_pairs_ends(['ACGT'], ['ACGT'], matrix=[int(x) for x in mat.reshape(-1)], alphabet='ACGT')
    with pytest.raises(ValueError, match='outside -128..127'):
        ssw_wrap.align_pairs_ends(['ACGT'], ['ACGT'], matrix=np.full((4, 4), 1e6), alphabet='ACGT')
    lim = np.array([[-128, 127], [127, -128]])
    assert ssw_wrap._int8_matrix(lim, 'x').tolist() == [-128, 127, 127, -128] and ssw_wrap._int8_matrix(lim, 'x').dtype == np.int8
    assert ssw_wrap._int8_matrix(ssw_wrap.BLOSUM62, 'x').tobytes() == ssw_wrap.BLOSUM62.tobytes()
