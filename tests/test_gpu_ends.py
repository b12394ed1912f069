"""End-anchored affine-gap alignment of pairs on the GPU (K1g, csrc/ssw_ends.hip): global, semiglobal, overlap.  Every expected
value is tests/ends_check.py; one case also compares with the existing GPU path, edlib.align_batch at unit costs.  Edge lengths
come from the plan's own geometry (EndsPlan.info), not from constants."""
import numpy as np
import pytest

import ends_check as chk

pytestmark = pytest.mark.gpu

MODES = chk.MODES
SCORINGS = [(2, 2, 3, 1), (10, 4, 8, 2), (1, 1, 1, 1)]


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


def _check_dna(refs, queries, mode, scoring):
    """align_pairs_ends against the checker, field by field; every CIGAR is also rescored on its own -> the results"""
    from ciri_long_amd import ssw_wrap
    ma, mi, go, ge = scoring
    got = ssw_wrap.align_pairs_ends(refs, queries, mode=mode, match=ma, mismatch=mi, gap_open=go, gap_extend=ge, report_cigar=True)
    assert len(got) == len(refs)
    mat = chk.dna_matrix(ma, mi)
    for k, (rs, qs, g) in enumerate(zip(refs, queries, got)):
        q, r = chk.encode(qs), chk.encode(rs)
        want = chk.align(q, r, mat, go, ge, mode)
        have = (g.score, g.ref_begin, g.ref_end, g.query_begin, g.query_end, g.cigar_string)
        assert have == chk.as_tuple(want)[:5] + (_text(want, len(qs)),), (k, mode, scoring, len(qs), len(rs))
        assert g.score2 is None and g.ref_end2 is None
        ops = [(o, n) for o, n in chk.parse_cigar(g.cigar_string) if o != 'S']
        chk.check_cigar(dict(score=g.score, ref_begin=g.ref_begin, ref_end=g.ref_end, query_begin=g.query_begin, query_end=g.query_end, cigar=ops),
                        q, r, mat, go, ge, mode)
    return got


@pytest.mark.parametrize('alpha', ['AC', 'ACGT'])
@pytest.mark.parametrize('mode', MODES)
def test_length_grid_around_the_chunk(geom, mode, alpha):
    C = geom['chunk']
    rng = chk.rng_for('gpu grid', mode, alpha)
    refs, queries = [], []
    for n in (1, 2, C - 1, C, C + 1, 2 * C + 1):
        for m in (1, 2, 3, 65):
            rs = chk.random_seq(rng, n, alpha)
            refs.append(rs); queries.append(chk.random_seq(rng, m, alpha))
            a = rng.randint(0, max(0, n - m))
            copy = chk.mutate(rng, rs[a:a + m], 0.10, alpha)
            refs.append(rs); queries.append((copy + chk.random_seq(rng, m, alpha))[:m])
    for scoring in SCORINGS:
        _check_dna(refs, queries, mode, scoring)


@pytest.mark.parametrize('ge', ['0', '1', 'go'])
def test_gaps_across_the_hand_over_between_chunks(geom, ge):
    C = geom['chunk']
    rng = chk.rng_for('hand-over', ge)
    go = 3
    scoring = (2, 2, go, {'0': 0, '1': 1, 'go': go}[ge])
    ref = chk.random_seq(rng, 3 * C)
    shorter = ref[:C - 70] + ref[C + 80:]                                  # 150 letters that straddle the first boundary are missing
    longer = ref[:2 * C] + chk.random_seq(rng, 150) + ref[2 * C:]           # 150 letters added at the second
    for mode in ('global', 'semiglobal'):
        got = _check_dna([ref, ref], [shorter, longer], mode, scoring)
        if scoring[3] < go:      # with ge == go one long gap costs what many short ones do, and the walk is free to scatter it
            assert '150D' in got[0].cigar_string and '150I' in got[1].cigar_string


def test_semiglobal_places_a_query_at_both_ends_in_the_middle_and_at_the_smaller_of_two_equal_columns(geom):
    rng = chk.rng_for('placements')
    probe = 'ACGGTCATTGCAAGTCCGATAGGCTTAACCGTGATCGGATATCCGGTAAC'
    assert len(probe) == 50
    base = list(chk.random_seq(rng, 2000, 'ACGT'))
    refs, at = [], [0, 977, 1950]
    for a in at:
        r = base[:]
        r[a:a + 50] = probe
        refs.append(''.join(r))
    twice = base[:]
    twice[300:350] = probe
    twice[1500:1550] = probe
    refs.append(''.join(twice))
    got = _check_dna(refs, [probe] * 4, 'semiglobal', (10, 4, 8, 2))
    for g, a in zip(got, at + [300]):
        assert (g.score, g.ref_begin, g.ref_end, g.cigar_string) == (500, a, a + 49, '50M')


def test_overlap_dovetails_containment_and_unrelated_sequences(geom):
    rng = chk.rng_for('overlap')
    s = chk.random_seq(rng, 120)
    x, y = chk.random_seq(rng, 700), chk.random_seq(rng, 450)
    refs = [x + s, s + x, x[:300] + s + x[300:], s, chk.random_seq(rng, 600, 'AC')]
    queries = [s + y, y + s, s, y[:200] + s + y[200:], chk.random_seq(rng, 40, 'GT')]
    got = _check_dna(refs, queries, 'overlap', (1, 3, 5, 2))       # scores under which unrelated flanks lose: the shared piece alone is best
    assert (got[0].score, got[0].ref_begin, got[0].ref_end, got[0].query_begin, got[0].query_end) == (120, 700, 819, 0, 119)
    assert (got[1].score, got[1].ref_begin, got[1].ref_end, got[1].query_begin, got[1].query_end) == (120, 0, 119, 450, 569)
    assert (got[2].score, got[2].ref_begin, got[2].query_begin, got[2].query_end) == (120, 300, 0, 119)
    assert (got[3].score, got[3].ref_begin, got[3].ref_end, got[3].query_begin) == (120, 0, 119, 200)
    _check_dna(refs, queries, 'overlap', (10, 4, 8, 2))
    u = got[4]           # no letter in common: the empty alignment at (m, 0)
    assert (u.score, u.ref_begin, u.ref_end, u.query_begin, u.query_end, u.cigar_string) == (0, 0, -1, 40, 39, '40S')


def test_spans_without_a_letter_alone_and_inside_a_batch(geom):
    rng = chk.rng_for('spans')
    table = {'semiglobal': (-14, 0, -1, 0, 3, '4I'), 'overlap': (0, 0, -1, 4, 3, '4S'), 'global': (-16, 0, 3, 0, 3, '4M')}
    others_r = [chk.random_seq(rng, n) for n in (30, 600, 7)]
    others_q = [chk.mutate(rng, r, 0.1)[:80] or 'A' for r in others_r]
    for mode, want in table.items():
        for refs, queries, k in ((['CCCC'], ['AAAA'], 0), (others_r[:2] + ['CCCC'] + others_r[2:], others_q[:2] + ['AAAA'] + others_q[2:], 2)):
            g = _check_dna(refs, queries, mode, (10, 4, 8, 2))[k]
            assert (g.score, g.ref_begin, g.ref_end, g.query_begin, g.query_end, g.cigar_string) == want, mode


def test_scores_below_the_int16_range_and_one_letter_against_forty_thousand(geom):
    from ciri_long_amd import ssw_wrap
    rng = chk.rng_for('below int16')
    rs, qs = chk.random_seq(rng, 3000), chk.random_seq(rng, 2900)
    mat = chk.dna_matrix(1, 30)
    want = chk.align(chk.encode(qs), chk.encode(rs), mat, 40, 20, 'global', path=False)
    assert want['score'] < -40000
    g = ssw_wrap.align_pairs_ends([rs], [qs], mode='global', match=1, mismatch=30, gap_open=40, gap_extend=20)[0]
    assert (g.score, g.ref_begin, g.ref_end, g.query_begin, g.query_end) == (want['score'], 0, 2999, 0, 2899)
    long_, one = chk.random_seq(rng, 40000), 'G'
    for mode in MODES:
        for r, q in ((long_, one), (one, long_)):
            w = chk.plain(chk.encode(q), chk.encode(r), mat, 40, 20, mode)
            g = ssw_wrap.align_pairs_ends([r], [q], mode=mode, match=1, mismatch=30, gap_open=40, gap_extend=20, report_cigar=True)[0]
            assert (g.score, g.ref_begin, g.ref_end, g.query_begin, g.query_end, g.cigar_string) == chk.as_tuple(w)[:5] + (_text(w, len(q)),), (mode, len(r))
    assert chk.plain(chk.encode(long_), chk.encode(one), mat, 40, 20, 'global')['score'] < -40000


@pytest.mark.parametrize('mode', MODES)
def test_blosum62_proteins_with_cigars(geom, mode):
    from ciri_long_amd import ssw_wrap
    rng = chk.rng_for('blosum', mode)
    letters = ssw_wrap.BLOSUM62_ALPHABET[:20]
    refs, queries = [], []
    for k in range(24):
        r = chk.random_seq(rng, rng.randint(50, 300), letters)
        q = chk.mutate(rng, r[rng.randint(0, 20):len(r) - rng.randint(0, 20)], 0.25, letters) if k & 1 else chk.random_seq(rng, rng.randint(50, 300), letters)
        refs.append(r); queries.append(q[:300] if len(q) >= 50 else q + chk.random_seq(rng, 50, letters))
    got = ssw_wrap.align_pairs_ends(refs, queries, mode=mode, gap_open=11, gap_extend=1, report_cigar=True, matrix=ssw_wrap.BLOSUM62,
                                    alphabet=ssw_wrap.BLOSUM62_ALPHABET)
    mat = ssw_wrap.BLOSUM62.astype(np.int64)
    for k, (rs, qs, g) in enumerate(zip(refs, queries, got)):
        q, r = chk.encode(qs, ssw_wrap.BLOSUM62_ALPHABET), chk.encode(rs, ssw_wrap.BLOSUM62_ALPHABET)
        want = chk.align(q, r, mat, 11, 1, mode)
        assert (g.score, g.ref_begin, g.ref_end, g.query_begin, g.query_end, g.cigar_string) == chk.as_tuple(want)[:5] + (_text(want, len(qs)),), k
        ops = [(o, n) for o, n in chk.parse_cigar(g.cigar_string) if o != 'S']
        chk.check_cigar(dict(score=g.score, ref_begin=g.ref_begin, ref_end=g.ref_end, query_begin=g.query_begin, query_end=g.query_end, cigar=ops),
                        q, r, mat, 11, 1, mode)


def test_a_code_outside_the_matrix_raises_and_names_the_pair(geom):
    from ciri_long_amd import hip, ssw_wrap
    ok = np.arange(20, dtype=np.int8)
    bad = ok.copy()
    bad[7] = 24
    with pytest.raises(hip.ClhError, match=r'pair 3: code 24 .* outside the matrix'):
        ssw_wrap.align_pairs_ends([ok] * 5, [ok, ok, ok, bad, bad], gap_open=11, gap_extend=1, matrix=ssw_wrap.BLOSUM62, alphabet=ssw_wrap.BLOSUM62_ALPHABET)
    with pytest.raises(hip.ClhError, match=r'pair 0: code -1 .* reference'):
        ssw_wrap.align_pairs_ends([np.array([0, -1], dtype=np.int8)], ['ACGT'])


def test_unit_costs_equal_edlib_align_batch_on_the_same_device(geom):
    from ciri_long_amd import edlib, ssw_wrap
    rng = chk.rng_for('edlib route')
    refs, queries = [], []
    for k in range(500):
        alpha = 'AC' if k % 5 == 0 else 'ACGT'
        r = chk.random_seq(rng, rng.randint(5, 300), alpha)
        q = chk.mutate(rng, r[rng.randint(0, len(r) // 2):], 0.12, alpha) if k & 1 else chk.random_seq(rng, rng.randint(1, 60), alpha)
        refs.append(r); queries.append(q or 'A')
    nw = edlib.align_batch(queries, refs, mode='NW', task='distance')
    hw = edlib.align_batch(queries, refs, mode='HW', task='distance')
    glob = ssw_wrap.align_pairs_ends(refs, queries, mode='global', match=0, mismatch=1, gap_open=1, gap_extend=1)
    semi = ssw_wrap.align_pairs_ends(refs, queries, mode='semiglobal', match=0, mismatch=1, gap_open=1, gap_extend=1)
    for k in range(500):
        assert (glob[k].score, glob[k].ref_end, glob[k].query_end) == (-nw[k]['editDistance'], len(refs[k]) - 1, len(queries[k]) - 1), k
        assert (semi[k].score, semi[k].ref_end) == (-hw[k]['editDistance'], hw[k]['locations'][0][1]), k


def _hip_rows(rows, cig):
    return [(int(r['score']), int(r['ref_begin']), int(r['ref_end']), int(r['query_begin']), int(r['query_end']),
             chk.cigar_text([('MID'[int(c) & 15], int(c) >> 4) for c in cig[int(r['cigar_off']):int(r['cigar_off']) + int(r['cigar_len'])]]))
            for r in rows]


def test_a_small_workspace_cuts_the_batch_and_one_pair_above_it_is_refused(geom):
    from ciri_long_amd import hip
    rng = chk.rng_for('workspace')
    refs = [chk.random_seq(rng, geom['chunk'] + 90) for _ in range(12)]
    queries = [chk.mutate(rng, r[50:260], 0.1) for r in refs]
    qd, qo = hip.pack(queries); rd, ro = hip.pack(refs)
    mat = hip.score_matrix(10, 4)
    ctx = _ctx()
    whole = ctx.ends_plan(qd, qo, rd, ro, mat, 8, 2, mode='semiglobal')
    try:
        per_pair = whole.info()['max_pair_bytes']
        assert whole.info()['shares'] == 1 and per_pair > 0
        whole.run()
        want = _hip_rows(*whole.fetch())
    finally:
        whole.close()
    cut = ctx.ends_plan(qd, qo, rd, ro, mat, 8, 2, mode='semiglobal', workspace_bytes=3 * per_pair + 8)
    try:
        info = cut.info()
        assert info['shares'] >= 3 and info['workspace_bytes'] <= 3 * per_pair + 8
        cut.run()
        assert _hip_rows(*cut.fetch()) == want
    finally:
        cut.close()
    cmat = chk.dna_matrix(10, 4)
    assert want == [chk.as_tuple(chk.align(chk.encode(q), chk.encode(r), cmat, 8, 2, 'semiglobal')) for q, r in zip(queries, refs)]
    with pytest.raises(hip.ClhError, match='workspace'):
        ctx.ends_plan(qd, qo, rd, ro, mat, 8, 2, mode='semiglobal', workspace_bytes=per_pair - 16)


@pytest.mark.parametrize('mode', MODES)
def test_one_plan_mixing_lengths_and_empty_sides_run_twice(geom, mode):
    from ciri_long_amd import hip
    rng = chk.rng_for('plan', mode)
    shapes = [(1, 1), (5000, 7), (0, 5), (7, 5000), (5, 0), (1200, 900), (0, 0), (64, geom['chunk']), (65, geom['chunk'] + 1), (2500, 100), (3, 2)]
    refs = [chk.random_seq(rng, n) for _, n in shapes]
    queries = [(chk.mutate(rng, r, 0.1) + chk.random_seq(rng, m))[:m] for (m, _), r in zip(shapes, refs)]
    assert [(len(q), len(r)) for q, r in zip(queries, refs)] == shapes
    qd, qo = hip.pack(queries); rd, ro = hip.pack(refs)
    plan = _ctx().ends_plan(qd, qo, rd, ro, hip.score_matrix(2, 2), 3, 1, mode=mode)
    try:
        assert plan.info()['empty_pairs'] == 3 and plan.info()['kernel_pairs'] == len(shapes) - 3
        plan.run()
        a = _hip_rows(*plan.fetch())
        plan.run()
        b = _hip_rows(*plan.fetch())
        assert plan.timing() > 0
    finally:
        plan.close()
    assert a == b
    mat = chk.dna_matrix(2, 2)
    for k, (q, r) in enumerate(zip(queries, refs)):
        assert a[k] == chk.as_tuple(chk.align(chk.encode(q), chk.encode(r), mat, 3, 1, mode)), (k, shapes[k])


def test_score_only_plans_leave_the_walk_out(geom):
    from ciri_long_amd import hip
    rng = chk.rng_for('score only')
    refs = [chk.random_seq(rng, n) for n in (40, geom['chunk'] + 33, 5, 0)]
    queries = [chk.mutate(rng, r, 0.1) or 'A' for r in refs[:3]] + ['ACG']
    qd, qo = hip.pack(queries); rd, ro = hip.pack(refs)
    mat = chk.dna_matrix(10, 4)
    for mode in MODES:
        rows, cig = _ctx().ends_batch(qd, qo, rd, ro, hip.score_matrix(10, 4), 8, 2, mode=mode, want_cigar=False)
        assert len(cig) == 0 and (rows['cigar_off'] == -1).all() and (rows['cigar_len'] == 0).all()
        for k, (q, r) in enumerate(zip(queries, refs)):
            w = chk.align(chk.encode(q), chk.encode(r), mat, 8, 2, mode)
            assert (int(rows[k]['score']), int(rows[k]['ref_end']), int(rows[k]['query_end'])) == (w['score'], w['ref_end'], w['query_end']), (mode, k)
            if mode == 'global' or not len(r):
                assert (int(rows[k]['ref_begin']), int(rows[k]['query_begin'])) == (w['ref_begin'], w['query_begin'])
            else:
                assert int(rows[k]['ref_begin']) == -1 and int(rows[k]['query_begin']) == (-1 if mode == 'overlap' else 0)


def test_refusals_carry_their_messages(geom):
    from ciri_long_amd import hip, ssw_wrap
    with pytest.raises(hip.ClhError, match=r'gap_open < gap_extend'):
        ssw_wrap.align_pairs_ends(['ACGT'], ['ACGT'], gap_open=1, gap_extend=2)
    with pytest.raises(hip.ClhError, match=r'pair 1: .*reaches 2\^30'):          # (4 + 4) 2^27 is the bound itself
        ssw_wrap.align_pairs_ends(['A', 'ACGT'], ['A', 'ACGT'], gap_open=1 << 27, gap_extend=0)
    ok = ssw_wrap.align_pairs_ends(['A', 'ACGT'], ['A', 'ACGT'], gap_open=(1 << 27) - 1, gap_extend=0)
    assert [g.score for g in ok] == [2, 8]
