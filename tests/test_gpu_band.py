"""Banded end-anchored alignment of pairs on the GPU (K1gb, csrc/ssw_band.hip): global and semiglobal over a band of diagonals.
Every expected value is tests/band_check.py, field by field and CIGAR by CIGAR; rows the band certifies (`exact`) are also compared
with K1g's full matrix on the same device (Context.ends_batch).  Widths come from the plan's own geometry (BandPlan.info), not from
constants.  Every case runs score-only and with CIGARs."""
import numpy as np
import pytest

import band_check as chk
import ends_check as ec

pytestmark = pytest.mark.gpu

SCORINGS = [(2, 2, 3, 1), (10, 4, 8, 2), (1, 1, 1, 1)]
OPS = 'MID'


def _ctx():
    from ciri_long_amd import hip
    return hip.default_context()


@pytest.fixture(scope='module')
def geom():
    from ciri_long_amd import hip
    plan = _ctx().band_plan(hip.encode('A'), [0, 1], hip.encode('A'), [0, 1], hip.score_matrix(2, 2), 3, 1, 0)
    try:
        g = plan.info()
    finally:
        plan.close()
    assert g['cpl'] == sorted(g['cpl']) and g['class_pairs'] == [1, 0, 0] and g['max_width'] == 1
    return g


def _class_of(geom, width):
    return min(c for c, cpl in enumerate(geom['cpl']) if width <= 64 * cpl)


def _rows(qs, rs, mat, go, ge, w, mode, diagonals=None, want_cigar=True, workspace_bytes=0, info=None):
    """Context.band_plan on sequences of codes -> one tuple per pair as band_check.as_tuple writes it (begins / cigar as the route gives them)"""
    from ciri_long_amd import hip
    qd, qo = hip.pack(qs); rd, ro = hip.pack(rs)
    plan = _ctx().band_plan(qd, qo, rd, ro, np.asarray(mat, dtype=np.int8).reshape(-1),      # row = reference code, as the checker's
                            go, ge, w, mode=mode, diagonals=diagonals, want_cigar=want_cigar, workspace_bytes=workspace_bytes)
    try:
        if info is not None:
            info.update(plan.info())
        plan.run()
        rows, cig = plan.fetch()
    finally:
        plan.close()
    out = []
    for r in rows:
        ops = None
        if want_cigar:
            ops = ''.join('%d%s' % (x >> 4, OPS[x & 15]) for x in cig[int(r['cigar_off']):int(r['cigar_off']) + int(r['cigar_len'])])
        else:
            assert r['cigar_off'] == -1 and r['cigar_len'] == 0
        out.append((int(r['score']), int(r['ref_begin']), int(r['ref_end']), int(r['query_begin']), int(r['query_end']), ops,
                    (int(r['band_lo']), int(r['band_hi'])), int(r['exact'])))
    return out


def _want(q, r, mat, go, ge, w, mode, diag=None):
    m, n = len(q), len(r)
    lo, hi = chk.band_of(m, n, w, diag)
    assert chk.refusal(mode, m, n, lo, hi) is None
    return chk.align(q, r, mat, go, ge, mode, lo, hi)


def _check(qs, rs, mat, go, ge, w, mode, diagonals=None, info=None, **kw):
    """both routes against the checker -> the checker's results"""
    qs = [np.asarray(q, dtype=np.int64) for q in qs]; rs = [np.asarray(r, dtype=np.int64) for r in rs]
    wants = [_want(q, r, mat, go, ge, w, mode, None if diagonals is None else diagonals[k]) for k, (q, r) in enumerate(zip(qs, rs))]
    got = _rows(qs, rs, mat, go, ge, w, mode, diagonals, True, info=info, **kw)
    bare = _rows(qs, rs, mat, go, ge, w, mode, diagonals, False)
    for k, want in enumerate(wants):
        assert got[k] == chk.as_tuple(want), (k, mode, (go, ge), w, len(qs[k]), len(rs[k]))
        if len(qs[k]) and len(rs[k]):
            chk.check_cigar(want, qs[k], rs[k], mat, go, ge, mode)
            begins = (0, 0) if mode == 'global' else (-1, 0)          # what the mode does not fix comes back as -1 without the walk
        else:
            begins = (got[k][1], got[k][3])
        assert bare[k] == (want['score'], begins[0], want['ref_end'], begins[1], want['query_end'], None, tuple(want['band']), want['exact']), (k, mode)
    return wants


def _dna(strings):
    return [chk.encode(s) for s in strings]


def _copy_of(rng, rs, m, rate=0.10):
    """a mutated copy of rs, cut or padded to m letters"""
    return (chk.mutate(rng, rs, rate) + chk.random_seq(rng, m))[:m]


WIDTHS = [(1, 0, 0), (2, 0, 1), (127, 63, 0), (128, 63, 1), (129, 64, 0), (255, 127, 0), (256, 127, 1), (257, 128, 0), (511, 255, 0), (512, 255, 1)]


@pytest.mark.parametrize('width,w,dn', WIDTHS, ids=[str(x[0]) for x in WIDTHS])
def test_clipped_widths_around_the_class_edges(geom, width, w, dn):
    rng = chk.rng_for('gpu band widths', width)
    m = 300
    rs = [chk.random_seq(rng, m + dn), chk.random_seq(rng, m + dn)]
    qs = [_copy_of(rng, rs[0], m), chk.random_seq(rng, m)]
    for ma, mi, go, ge in SCORINGS:
        info = {}
        wants = _check(_dna(qs), _dna(rs), chk.dna_matrix(ma, mi), go, ge, w, 'global', info=info)
        assert all(x['band'][1] - x['band'][0] + 1 == width for x in wants)
        assert info['max_width'] == width
        assert info['class_pairs'] == [2 if c == _class_of(geom, width) else 0 for c in range(3)]


def test_a_band_one_diagonal_above_the_widest_class_is_refused_and_names_the_pair(geom):
    from ciri_long_amd import hip, ssw_wrap
    top = 64 * geom['cpl'][-1]
    rng = chk.rng_for('gpu band 513')
    a, b = chk.random_seq(rng, 100), chk.random_seq(rng, 300)
    assert top % 2 == 0
    with pytest.raises(hip.ClhError, match=r'pair 1: the clipped band \[-%d, %d\] holds %d diagonals.*full matrix' % (top // 2, top // 2, top + 1)):
        ssw_wrap.align_pairs_band([a, b], [a, b], top // 2)
    ok = ssw_wrap.align_pairs_band([a, b + 'A'], [a, b], top // 2 - 1)
    assert ok[1].band == (-(top // 2 - 1), top // 2) and ok[0].band == (-100, 100)


@pytest.mark.parametrize('wide', [False, True], ids=['narrow', 'widest class'])
def test_rows_around_the_64_row_reload_of_the_letters(geom, wide):
    rng = chk.rng_for('gpu band rows', wide)
    top = 64 * geom['cpl'][-1]
    for mode in chk.MODES:
        # global: the corner diagonals 0 and n - m = 9 widened to the widest class (the matrix clips the band of a short pair);
        # semiglobal: a hint in a long reference, so that the band keeps its width whatever the number of rows
        w = 3 if not wide else ((top - 10) // 2 if mode == 'global' else top // 2 - 1)
        qs, rs = [], []
        for m in (1, 2, 63, 64, 65, 129):
            n = m + (5 if not wide else (9 if mode == 'global' else top + 18))
            r = chk.random_seq(rng, n)
            at = 0 if mode == 'global' else w
            rs.append(r); qs.append(_copy_of(rng, r[at:], m))
            rs.append(r[:m + 2]); qs.append(_copy_of(rng, r, m))
        for ma, mi, go, ge in SCORINGS:
            info = {}
            if mode == 'global':
                _check(_dna(qs), _dna(rs), chk.dna_matrix(ma, mi), go, ge, w, mode, info=info)
            else:
                _check(_dna(qs), _dna(rs), chk.dna_matrix(ma, mi), go, ge, w, mode, diagonals=[w if k % 2 == 0 else 0 for k in range(len(qs))], info=info)
            if wide:
                assert info['class_pairs'][-1] > 0


def test_bands_clipped_to_the_whole_matrix_are_exact_and_equal_the_full_matrix_kernel():
    from ciri_long_amd import hip
    rng = chk.rng_for('gpu band clipped')
    qs, rs = [], []
    for m, n in ((1, 1), (1, 40), (40, 1), (1, 1), (1, 40), (40, 1)):
        rs.append(chk.random_seq(rng, n, 'AC')); qs.append(chk.random_seq(rng, m, 'AC'))
    for ma, mi, go, ge in SCORINGS:
        for mode in chk.MODES:
            wants = _check(_dna(qs), _dna(rs), chk.dna_matrix(ma, mi), go, ge, 64, mode)
            assert all(x['exact'] == 1 and x['band'] == (-len(q), len(r)) for x, q, r in zip(wants, qs, rs))
            qd, qo = hip.pack(qs); rd, ro = hip.pack(rs)
            rows, cig = _ctx().ends_batch(qd, qo, rd, ro, hip.score_matrix(ma, mi), go, ge, mode=mode)
            for k, x in enumerate(wants):
                r = rows[k]
                ops = ''.join('%d%s' % (v >> 4, OPS[v & 15]) for v in cig[int(r['cigar_off']):int(r['cigar_off']) + int(r['cigar_len'])])
                assert (int(r['score']), int(r['ref_begin']), int(r['ref_end']), int(r['query_begin']), int(r['query_end']), ops) == ec.as_tuple(x)


def test_cigars_with_as_many_runs_as_the_host_reserves():
    """the walk over half-bytes in the band's frame writes its last run at nops == cig_cap - 1: the one-piece K1g checker's rows,
    over a band that clips to the whole matrix (the widest pair spans 156 diagonals)"""
    import ends_edges as E
    from ciri_long_amd import ssw_wrap
    refs, queries, _ = E.max_runs_rows(E.HOST_GEOM)
    ma, mi, go, ge = E.MAX_RUNS_SCORING
    got = ssw_wrap.align_pairs_band(refs, queries, 128, mode='global', match=ma, mismatch=mi, gap_open=go, gap_extend=ge, report_cigar=True)
    E.check_max_runs(got, E.HOST_GEOM)
    assert all(g.band_exact for g in got)


@pytest.mark.parametrize('ge', ['2', '0', 'go'])
def test_gaps_of_exactly_the_half_width_touch_hi_then_lo_and_one_less_loses_them(ge):
    rng = chk.rng_for('gpu band edge gaps', ge)
    w, go = 40, 8
    scoring = (10, 4, go, {'2': 2, '0': 0, 'go': go}[ge])
    ref = chk.random_seq(rng, 400)
    cut = ref[:100] + ref[100 + w:]                               # a deletion of exactly w letters: the path runs on diagonal hi
    qry = cut[:200] + chk.random_seq(rng, w) + cut[200:]          # then an insertion of exactly w: it comes back to lo + w = 0
    mat = chk.dna_matrix(scoring[0], scoring[1])
    full = ec.align(chk.encode(qry), chk.encode(ref), mat, scoring[2], scoring[3], 'global')
    at, = _check(_dna([qry]), _dna([ref]), mat, scoring[2], scoring[3], w, 'global')
    below, = _check(_dna([qry]), _dna([ref]), mat, scoring[2], scoring[3], w - 1, 'global')
    assert at['score'] == full['score']
    if scoring[3] < go:      # with ge == go a long gap costs what many short ones do: the best alignment scatters it and never nears the edge
        assert below['score'] < full['score'] and below['exact'] == 0
        assert '%dD' % w in ec.cigar_text(at['cigar']) and '%dI' % w in ec.cigar_text(at['cigar'])
        assert max(j - i for i, j in chk.cells_of(at)) == w and ec.as_tuple(at) == ec.as_tuple(full)


def test_the_zigzag_pair_at_29_and_30():
    from test_band_host import zigzag
    qs, rs = zigzag()
    mat = chk.dna_matrix(10, 4)
    narrow, = _check(_dna([qs]), _dna([rs]), mat, 8, 2, 29, 'global')
    wide, = _check(_dna([qs]), _dna([rs]), mat, 8, 2, 30, 'global')
    assert narrow['exact'] == 0 and wide['exact'] == 1 and narrow['score'] < wide['score']


def test_semiglobal_placements_with_hints_near_and_far():
    from ciri_long_amd import hip, ssw_wrap
    rng = chk.rng_for('gpu band placements')
    probe = chk.random_seq(rng, 50)
    base = chk.random_seq(rng, 2000)
    mat = chk.dna_matrix(10, 4)
    qs, rs, diags, truth = [], [], [], []
    for at in (0, 977, 1950):
        ref = base[:at] + probe + base[at + 50:]
        q = _copy_of(rng, probe, 50)
        for off in (0, 7, 8, 9, None):
            d = 0 if off is None else (at + off if at < 1000 else at - off)
            qs.append(q); rs.append(ref); diags.append(d); truth.append(at)
    keep = [k for k in range(len(qs)) if chk.refusal('semiglobal', 50, 2000, diags[k] - 8, diags[k] + 8) is None]
    assert len(keep) == len(qs)
    wants = _check(_dna(qs), _dna(rs), mat, 8, 2, 8, 'semiglobal', diagonals=diags)
    full = [ec.align(chk.encode(q), chk.encode(r), mat, 8, 2, 'semiglobal') for q, r in zip(qs[::5], rs[::5])]
    for g in range(3):
        assert ec.as_tuple(wants[5 * g]) == ec.as_tuple(full[g])                       # the true diagonal reproduces the unbanded placement
        assert full[g]['score'] > 300
        far = [k for k in range(5 * g, 5 * g + 5) if abs(diags[k] - truth[k]) > 20]
        assert all(wants[k]['score'] < full[g]['score'] for k in far) and (far or truth[5 * g] == 0)
        assert all(x['exact'] == 0 for x in wants[5 * g:5 * g + 5])
    # the wrapper: text in, text out, hints as a list
    got = ssw_wrap.align_pairs_band(rs, qs, 8, mode='semiglobal', diagonals=diags, match=10, mismatch=4, gap_open=8, gap_extend=2, report_cigar=True)
    for g, x in zip(got, wants):
        assert (g.score, g.ref_begin, g.ref_end, g.query_begin, g.query_end, g.band, g.band_exact) == ec.as_tuple(x)[:5] + (tuple(x['band']), bool(x['exact']))
        assert g.cigar_string == ec.cigar_text(x['cigar']) and g.score2 is None
    # refusals: no start cell, no end cell, and a global hint that misses a corner
    with pytest.raises(hip.ClhError, match=r'pair 1: the band \[-20, -4\] of the 50 x 2000 pair has no start cell'):
        ssw_wrap.align_pairs_band(rs[:2], qs[:2], 8, mode='semiglobal', diagonals=[0, -12])
    with pytest.raises(hip.ClhError, match=r'pair 0: the band \[1951, 1967\] .* no end cell .*n - m = 1950'):
        ssw_wrap.align_pairs_band(rs[:2], qs[:2], 8, mode='semiglobal', diagonals=[1959, 0])
    with pytest.raises(hip.ClhError, match=r'pair 0: the band \[1, 17\] of the 50 x 2000 pair misses \(0, 0\) or \(m, n\)'):
        ssw_wrap.align_pairs_band(rs[:1], qs[:1], 8, mode='global', diagonals=[9])
    with pytest.raises(hip.ClhError, match=r'overlap with a band is not built'):
        _ctx().band_plan(hip.encode('A'), [0, 1], hip.encode('A'), [0, 1], hip.score_matrix(2, 2), 3, 1, 4, mode='overlap')
    with pytest.raises(hip.ClhError, match=r'gap_open < gap_extend'):
        ssw_wrap.align_pairs_band(['ACGT'], ['ACGT'], 4, gap_open=1, gap_extend=2)
    with pytest.raises(hip.ClhError, match=r'pair 1: code 9 at letter 2 of the query is outside the matrix'):
        ssw_wrap.align_pairs_band(['ACGT', 'ACGT'], ['ACGT', np.array([0, 1, 9], dtype=np.int8)], 4)


def test_a_pair_the_full_matrix_refuses_runs_in_the_same_workspace():
    from ciri_long_amd import hip
    rng = chk.rng_for('gpu band 3000')
    ref = chk.random_seq(rng, 3000)
    qry = _copy_of(rng, ref, 3000)
    mat = chk.dna_matrix(10, 4)
    qd, qo = hip.pack([qry]); rd, ro = hip.pack([ref])
    with pytest.raises(hip.ClhError, match=r'pair 0 alone needs 4[0-9]{6} bytes'):
        _ctx().ends_plan(qd, qo, rd, ro, hip.score_matrix(10, 4), 8, 2, mode='global', workspace_bytes=1 << 20)
    info = {}
    want, = _check(_dna([qry]), _dna([ref]), mat, 8, 2, 32, 'global', info=info, workspace_bytes=1 << 20)
    assert info['shares'] == 1 and info['max_pair_bytes'] <= 3000 * 66 // 2 + 16 and want['score'] > 15000


def test_workspace_shares_and_the_pair_above_the_workspace():
    from ciri_long_amd import hip
    rng = chk.rng_for('gpu band shares')
    rs = [chk.random_seq(rng, 200) for _ in range(12)]
    qs = [_copy_of(rng, r, 200) for r in rs]
    mat = chk.dna_matrix(10, 4)
    one = {}
    _check(_dna(qs[:1]), _dna(rs[:1]), mat, 8, 2, 20, 'global', info=one)
    per_pair = one['max_pair_bytes']
    assert per_pair >= 200 * 41 // 2 and one['workspace_bytes'] == per_pair
    whole, cut = {}, {}
    a = _check(_dna(qs), _dna(rs), mat, 8, 2, 20, 'global', info=whole)
    b = _check(_dna(qs), _dna(rs), mat, 8, 2, 20, 'global', info=cut, workspace_bytes=3 * per_pair + 8)
    assert whole['shares'] == 1 and cut['shares'] >= 3 and cut['workspace_bytes'] <= 3 * per_pair + 8
    assert [chk.as_tuple(x) for x in a] == [chk.as_tuple(x) for x in b]
    qd, qo = hip.pack(qs); rd, ro = hip.pack(rs)
    with pytest.raises(hip.ClhError, match=r'pair 0 alone needs %d bytes of workspace .* 200 rows of 41 diagonals' % per_pair):
        _ctx().band_plan(qd, qo, rd, ro, hip.score_matrix(10, 4), 8, 2, 20, workspace_bytes=per_pair - 16)


def test_one_plan_run_twice_mixes_the_classes_and_empty_and_one_letter_sides(geom):
    from ciri_long_amd import hip
    rng = chk.rng_for('gpu band twice')
    shapes = [(300, 300), (0, 0), (300, 340), (1, 1), (0, 7), (300, 420), (7, 0), (1, 90), (90, 1), (300, 301), (300, 700)]
    rs = [chk.random_seq(rng, n) for _, n in shapes]
    qs = [_copy_of(rng, r, m) if m else '' for (m, _), r in zip(shapes, rs)]
    mat = chk.dna_matrix(2, 2)
    for mode in chk.MODES:
        w = 40
        ok = [k for k, (m, n) in enumerate(shapes) if chk.refusal(mode, m, n, *chk.band_of(m, n, w)) is None]
        q2, r2 = [qs[k] for k in ok], [rs[k] for k in ok]
        info = {}
        wants = _check(_dna(q2), _dna(r2), mat, 3, 1, w, mode, info=info)
        assert info['empty_pairs'] == 3 and all(c > 0 for c in info['class_pairs']) and sum(info['class_pairs']) == len(ok) - 3
        qd, qo = hip.pack(q2); rd, ro = hip.pack(r2)
        plan = _ctx().band_plan(qd, qo, rd, ro, hip.score_matrix(2, 2), 3, 1, w, mode=mode)
        try:
            plan.run(); first = plan.fetch()
            assert plan.timing() > 0
            plan.run(); second = plan.fetch()
        finally:
            plan.close()
        assert first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes()
        assert [int(x) for x in first[0]['score']] == [x['score'] for x in wants]


def test_blosum62_global_with_cigars_rescored():
    from ciri_long_amd import ssw_wrap
    rng = chk.rng_for('gpu band blosum')
    alpha = ssw_wrap.BLOSUM62_ALPHABET
    mat = np.asarray(ssw_wrap.BLOSUM62, dtype=np.int64)
    qs, rs = [], []
    for k in range(24):
        r = chk.random_seq(rng, rng.randint(50, 300), alpha[:20])
        q = chk.mutate(rng, r, 0.10, alpha[:20])
        q = q[:len(r) + 20] or r
        rs.append(r); qs.append(q)
    enc = lambda s: np.array([alpha.index(c) for c in s], dtype=np.int64)
    wants = _check([enc(q) for q in qs], [enc(r) for r in rs], mat, 11, 1, 24, 'global')
    got = ssw_wrap.align_pairs_band(rs, qs, 24, gap_open=11, gap_extend=1, report_cigar=True, matrix=ssw_wrap.BLOSUM62, alphabet=alpha)
    for g, x, q, r in zip(got, wants, qs, rs):
        assert (g.score, g.cigar_string, g.band_exact) == (x['score'], ec.cigar_text(x['cigar']), bool(x['exact']))
        score, nr, nq = ec.rescore(ec.parse_cigar(g.cigar_string), enc(q), enc(r), 0, 0, mat, 11, 1)
        assert (score, nr, nq) == (g.score, len(r), len(q))


def exact_set():
    """200 global pairs: 300-letter references with 10 % mutated copies, half at w = 16 and half at w = 32"""
    rng = chk.rng_for('gpu band exact')
    rs = [chk.random_seq(rng, 300) for _ in range(200)]
    qs = [chk.mutate(rng, r, 0.10) for r in rs]
    return qs, rs


def test_the_exact_flag_on_the_device_and_certified_rows_equal_the_full_matrix_kernel():
    from ciri_long_amd import hip
    qs, rs = exact_set()
    mat = chk.dna_matrix(10, 4)
    wants = _check(_dna(qs[:100]), _dna(rs[:100]), mat, 8, 2, 16, 'global') + _check(_dna(qs[100:]), _dna(rs[100:]), mat, 8, 2, 32, 'global')
    n1 = sum(x['exact'] for x in wants)
    print('exact on the device: %d of 200 certified (%d at w = 16, %d at w = 32)' % (n1, sum(x['exact'] for x in wants[:100]), sum(x['exact'] for x in wants[100:])))
    assert n1 >= 40 and 200 - n1 >= 40                                   # at least a fifth of the pairs of each kind
    qd, qo = hip.pack(qs); rd, ro = hip.pack(rs)
    rows, cig = _ctx().ends_batch(qd, qo, rd, ro, hip.score_matrix(10, 4), 8, 2, mode='global')
    for k, x in enumerate(wants):
        if x['exact']:
            r = rows[k]
            ops = ''.join('%d%s' % (v >> 4, OPS[v & 15]) for v in cig[int(r['cigar_off']):int(r['cigar_off']) + int(r['cigar_len'])])
            assert (int(r['score']), int(r['ref_begin']), int(r['ref_end']), int(r['query_begin']), int(r['query_end']), ops) == ec.as_tuple(x), k


def test_score_bound_last_value_below_runs_and_the_bound_itself_is_refused(geom):
    from ciri_long_amd import hip, ssw_wrap
    span = 4 + 4 + 2 * 64 * geom['cpl'][-1]
    go = ((1 << 29) - 1) // span                                          # (m + n + 1024) go < 2^29 <= (m + n + 1024) (go + 1)
    assert span * go < (1 << 29) <= span * (go + 1)
    q, r = 'ACGT', 'AGGT'
    for ge in (0, go):
        for mode in chk.MODES:
            want, = _check(_dna(['A', q]), _dna(['A', r]), chk.dna_matrix(2, 2), go, ge, 1, mode)[1:]
            assert want['score'] == 4
    with pytest.raises(hip.ClhError, match=r'pair 1: \(m \+ n \+ %d\) \* max\(\|s\|, gap_open, gap_extend\) = %d \* %d reaches 2\^29' % (span - 8, span, go + 1)):
        ssw_wrap.align_pairs_band(['A', r], ['A', q], 1, gap_open=go + 1, gap_extend=0)
