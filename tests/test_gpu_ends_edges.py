"""The end-anchored alignment kernels (K1g, csrc/ssw_ends.hip) on the edge sets of tests/ends_edges.py: every case field by field
against tests/ends_check.py, every CIGAR rescored on its own, and every set a second time without CIGARs (the STORE = false
instantiations).  tests/test_ends_edges_host.py proves on the CPU that the sets reach the edges they are named for; the lengths here
come from the plan's own geometry (EndsPlan.info)."""
import numpy as np
import pytest

import ends_check as chk
import ends_edges as E

pytestmark = pytest.mark.gpu

MODES = chk.MODES


def _ctx():
    from ciri_long_amd import hip
    return hip.default_context()


@pytest.fixture(scope='module')
def geom():
    from ciri_long_amd import hip
    plan = _ctx().ends_plan(hip.encode('A'), [0, 1], hip.encode('A'), [0, 1], hip.score_matrix(2, 2), 3, 1)
    try:
        g = plan.info()
    finally:
        plan.close()
    assert g['cpl'] >= 1 and g['chunk'] == 64 * g['cpl']
    return g


def _text(want, m):
    """the cigar_string of a checker result: soft clips around the ops, as PyAlignRes writes them"""
    head = '%dS' % want['query_begin'] if want['query_begin'] > 0 else ''
    tail = m - want['query_end'] - 1
    return head + chk.cigar_text(want['cigar']) + ('%dS' % tail if tail else '')


def _groups(cases):
    """cases of one scoring and mode go to the device in one call, in the order of the set"""
    out = {}
    for c in cases:
        out.setdefault(E.scoring_key(c), []).append(c)
    return list(out.values())


def _device_scoring(case):
    """-> (int8 matrix for the plan, encoder of a sequence)"""
    from ciri_long_amd import hip, ssw_wrap
    if case.alphabet is None:
        return hip.score_matrix(*case.scoring), hip.encode
    return np.ascontiguousarray(case.scoring, dtype=np.int8), lambda s: ssw_wrap.encode_alphabet(s, case.alphabet)


def _check(cases):
    """align_pairs_ends(report_cigar=True) against the checker, field by field, every CIGAR also rescored on its own; then the same
    cases through ends_batch without CIGARs: score and ends equal, begins as a plan without a walk states them -> the results"""
    from ciri_long_amd import hip, ssw_wrap
    assert cases, 'a set without a case'
    results = []
    for group in _groups(cases):
        c0 = group[0]
        refs, queries = [c.ref for c in group], [c.query for c in group]
        kw = dict(match=c0.scoring[0], mismatch=c0.scoring[1]) if c0.alphabet is None else dict(matrix=c0.scoring, alphabet=c0.alphabet)
        got = ssw_wrap.align_pairs_ends(refs, queries, mode=c0.mode, gap_open=c0.go, gap_extend=c0.ge, report_cigar=True, **kw)
        assert len(got) == len(group)
        mat = E.matrix_of(c0)
        wants = []
        for k, (c, g) in enumerate(zip(group, got)):
            q, r = E.codes_of(c)
            want = E.expected(c)
            wants.append(want)
            have = (g.score, g.ref_begin, g.ref_end, g.query_begin, g.query_end, g.cigar_string)
            assert have == chk.as_tuple(want)[:5] + (_text(want, len(q)),), (k, c.mode, c.go, c.ge, len(q), len(r))
            assert g.score2 is None and g.ref_end2 is None
            ops = [(o, n) for o, n in chk.parse_cigar(g.cigar_string) if o != 'S']
            chk.check_cigar(dict(score=g.score, ref_begin=g.ref_begin, ref_end=g.ref_end, query_begin=g.query_begin, query_end=g.query_end, cigar=ops),
                            q, r, mat, c.go, c.ge, c.mode)
        dmat, enc = _device_scoring(c0)
        qd, qo = hip.pack([enc(s) for s in queries]); rd, ro = hip.pack([enc(s) for s in refs])
        rows, cig = _ctx().ends_batch(qd, qo, rd, ro, dmat, c0.go, c0.ge, mode=c0.mode, want_cigar=False)
        assert len(rows) == len(group) and len(cig) == 0 and (rows['cigar_off'] == -1).all() and (rows['cigar_len'] == 0).all()
        for k, (c, w) in enumerate(zip(group, wants)):
            assert (int(rows[k]['score']), int(rows[k]['ref_end']), int(rows[k]['query_end'])) == (w['score'], w['ref_end'], w['query_end']), (k, c.mode)
            if c.mode == 'global' or not len(c.ref):
                assert (int(rows[k]['ref_begin']), int(rows[k]['query_begin'])) == (w['ref_begin'], w['query_begin']), (k, c.mode)
            else:
                assert int(rows[k]['ref_begin']) == -1 and int(rows[k]['query_begin']) == (-1 if c.mode == 'overlap' else 0), (k, c.mode)
        results += got
    assert len(results) == len(cases)
    return results


def _of_mode(name, geom, mode):
    cases = [c for c in E.SETS[name](geom) if c.mode == mode]
    assert cases, (name, mode)
    return cases


@pytest.mark.parametrize('mode', MODES)
def test_asymmetric_matrices_of_2_to_32_letters(geom, mode):
    cases = _of_mode('asymmetric', geom, mode)
    assert len({c.scoring.tobytes() for c in cases}) == 5
    _check(cases)


@pytest.mark.parametrize('mode', MODES)
def test_queries_around_the_row_blocks_with_several_chunks(geom, mode):
    cases = _of_mode('row blocks', geom, mode)
    got = _check(cases)
    planted = [g for c, g in zip(cases, got) if (c.ref, c.query) == E.planted_insertion(geom)]
    assert len(planted) == 1 and any(o == 'I' and n >= 70 for o, n in chk.parse_cigar(planted[0].cigar_string))


@pytest.mark.parametrize('mode', MODES)
def test_column_n_in_every_register_and_lane_count(geom, mode):
    cases = _of_mode('column geometry', geom, mode)
    assert {(len(c.ref) - 1) % geom['cpl'] for c in cases} == set(range(geom['cpl']))
    _check(cases)


def test_overlap_end_cells_at_exact_ties(geom):
    named = E.overlap_ends(geom)
    got = _check([c for _, c in named])
    for (name, c), g in zip(named, got):
        m, n = len(c.query), len(c.ref)
        if name == 'row ties column':
            assert (g.score, g.ref_begin, g.ref_end, g.query_begin, g.query_end) == (40, 0, 39, m - 40, m - 1)
        elif name == 'column above row':
            assert (g.score, g.ref_begin, g.ref_end, g.query_begin, g.query_end) == (41, n - 41, n - 1, 0, 40)
        elif name == 'two in the last column':
            assert (g.score, g.ref_begin, g.ref_end, g.query_begin, g.query_end) == (n, 0, n - 1, 10, 10 + n - 1)
        elif name == 'two in the last row':
            assert (g.score, g.ref_begin, g.ref_end, g.query_begin, g.query_end) == (m, 100, 100 + m - 1, 0, m - 1)
        elif name == 'nothing in common':
            assert (g.score, g.ref_begin, g.ref_end, g.query_begin, g.query_end, g.cigar_string) == (0, 0, -1, m, m - 1, '%dS' % m)
        else:
            i = int(name.split()[-1])
            assert (g.score, g.ref_end, g.query_end) == (min(i, n), n - 1, i - 1), name


@pytest.mark.parametrize('mode', MODES)
def test_gap_costs_under_which_almost_every_cell_is_a_tie(geom, mode):
    cases = _of_mode('gap corners', geom, mode)
    assert {(c.go, c.ge) for c in cases} == {(0, 0), (3, 0), (7, 7), (3, 1)}
    _check(cases)


@pytest.mark.parametrize('mode', MODES)
def test_the_int32_frame_one_below_the_hosts_bound_and_the_refusal_at_it(geom, mode):
    from ciri_long_amd import hip, ssw_wrap
    cases = _of_mode('int32 frame', geom, mode)
    big = E.frame_limit(geom)
    assert {(c.go, c.ge) for c in cases} == {(big, big), (big, 1)}
    got = _check(cases)                                     # the accepted neighbour equals the checker
    if mode == 'global':
        assert min(g.score for g in got) < -(1 << 29)
    (ref, qry), _ = E.frame_pairs(geom)
    with pytest.raises(hip.ClhError, match=r'pair 1: \(m \+ n\) \* max\(\|s\|, gap_open, gap_extend\) = %d \* %d reaches 2\^30' % (len(ref) + len(qry), big + 1)):
        ssw_wrap.align_pairs_ends(['ACGT', ref], ['ACGT', qry], mode=mode, gap_open=big + 1, gap_extend=1, report_cigar=True)


def test_cigars_with_as_many_runs_as_the_host_reserves(geom):
    cases = E.SETS['max runs'](geom)
    got = _check(cases)
    for c, g in zip(cases, got):
        assert len(chk.parse_cigar(g.cigar_string)) == E.run_capacity(len(c.query), len(c.ref)), (c.ref, c.query, g.cigar_string)
    assert got[0].cigar_string == '2D1M3D1M2D'


def _hip_rows(rows, cig):
    return [(int(r['score']), int(r['ref_begin']), int(r['ref_end']), int(r['query_begin']), int(r['query_end']),
             chk.cigar_text([('MID'[int(c) & 15], int(c) >> 4) for c in cig[int(r['cigar_off']):int(r['cigar_off']) + int(r['cigar_len'])]]))
            for r in rows]


@pytest.mark.parametrize('mode', E.SHARES_MODES)
def test_shares_of_unequal_pairs_at_the_smallest_workspace_in_both_orders(geom, mode):
    from ciri_long_amd import hip
    ma, mi, go, ge = E.SHARES_SCORING
    cmat = chk.dna_matrix(ma, mi)
    ctx = _ctx()
    given = E.shares_pairs(geom)
    for pairs in (given, given[::-1]):
        refs, queries = [r for r, _ in pairs], [q for _, q in pairs]
        shapes = [(len(q), len(r)) for r, q in pairs]
        large = sum(1 for m, n in shapes if n > geom['chunk'] and m > 64)
        assert large == 2
        want = [chk.as_tuple(chk.align(chk.encode(q), chk.encode(r), cmat, go, ge, mode)) for r, q in pairs]
        qd, qo = hip.pack(queries); rd, ro = hip.pack(refs)
        top = max(E.pair_workspace_bytes(m, n, geom) for m, n in shapes if m and n)
        for ws in E.SHARES_WORKSPACES:
            bytes_ = {'default': 0, 'max_pair_bytes': top, 'max_pair_bytes + 16': top + 16}[ws]
            plan = ctx.ends_plan(qd, qo, rd, ro, hip.score_matrix(ma, mi), go, ge, mode=mode, workspace_bytes=bytes_)
            try:
                info = plan.info()
                assert info['max_pair_bytes'] == top and info['empty_pairs'] == 2 and info['kernel_pairs'] == 7
                if ws == 'default':
                    assert info['shares'] == 1
                else:
                    assert info['shares'] == E.share_count(shapes, bytes_, geom) > 1 and info['workspace_bytes'] <= bytes_
                    if ws == 'max_pair_bytes':
                        assert info['shares'] >= large + 1           # each large pair alone, and the small ones elsewhere
                plan.run()
                assert _hip_rows(*plan.fetch()) == want, (ws, pairs is given)
            finally:
                plan.close()
        with pytest.raises(hip.ClhError, match='workspace'):
            ctx.ends_plan(qd, qo, rd, ro, hip.score_matrix(ma, mi), go, ge, mode=mode, workspace_bytes=top - 16)
        rows, cig = ctx.ends_batch(qd, qo, rd, ro, hip.score_matrix(ma, mi), go, ge, mode=mode, want_cigar=False)
        assert len(cig) == 0
        assert [(int(r['score']), int(r['ref_end']), int(r['query_end'])) for r in rows] == [(w[0], w[2], w[4]) for w in want]
