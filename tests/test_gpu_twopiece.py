"""Two-piece affine gap costs on the GPU: K1g (csrc/ssw_ends.hip), all five modes over the full matrix, and K1gb (csrc/ssw_band.hip),
four modes over a band.  Every expected value is tests/twopiece_check.py, field by field with CIGARs, through the storing route and
the score-only route; rows a band certifies are also held to the two-piece K1g rows of the same device."""
import numpy as np
import pytest

import ends_check as ec
import twopiece_check as chk

pytestmark = pytest.mark.gpu

MODES = chk.MODES
LONG = (4, 2, 24, 1)            # at match 2, mismatch 4: the pieces swap at 22 letters


def _ctx():
    from ciri_long_amd import hip
    return hip.default_context()


def _text(want, m):
    head = '%dS' % want['query_begin'] if want['query_begin'] > 0 else ''
    tail = m - want['query_end'] - 1
    return head + chk.cigar_text(want['cigar']) + ('%dS' % tail if tail else '')


def _hip_rows(rows, cig):
    return [(int(r['score']), int(r['ref_begin']), int(r['ref_end']), int(r['query_begin']), int(r['query_end']),
             chk.cigar_text([('MID'[int(c) & 15], int(c) >> 4) for c in cig[int(r['cigar_off']):int(r['cigar_off']) + int(r['cigar_len'])]]))
            for r in rows]


def _check(refs, queries, mode, costs, match=2, mismatch=4, wants=None, matrix=None, alphabet=None):
    """align_pairs_ends with two pieces against the checker, field by field, storing route and score-only route; every CIGAR is
    also rescored on its own -> the checker's results"""
    from ciri_long_amd import hip, ssw_wrap
    kw = dict(mode=mode, gap_open=costs[0], gap_extend=costs[1], gap_open2=costs[2], gap_extend2=costs[3])
    if matrix is None:
        kw.update(match=match, mismatch=mismatch)
        mat = chk.dna_matrix(match, mismatch)
        enc = chk.encode
    else:
        kw.update(matrix=matrix, alphabet=alphabet)
        mat = np.asarray(matrix, dtype=np.int64)
        enc = lambda s: chk.encode(s, alphabet)
    got = ssw_wrap.align_pairs_ends(refs, queries, report_cigar=True, **kw)
    assert len(got) == len(refs)
    if wants is None:
        wants = [chk.align(enc(qs), enc(rs), mat, costs, mode) for rs, qs in zip(refs, queries)]
    for k, (rs, qs, g, want) in enumerate(zip(refs, queries, got, wants)):
        have = (g.score, g.ref_begin, g.ref_end, g.query_begin, g.query_end, g.cigar_string)
        assert have == chk.as_tuple(want)[:5] + (_text(want, len(qs)),), (k, mode, costs, len(qs), len(rs))
        ops = [(o, n) for o, n in chk.parse_cigar(g.cigar_string) if o != 'S']
        chk.check_cigar(dict(score=g.score, ref_begin=g.ref_begin, ref_end=g.ref_end, query_begin=g.query_begin, query_end=g.query_end, cigar=ops),
                        enc(qs), enc(rs), mat, costs, mode)
    # the score-only route: another instantiation of the kernel, no stored decisions, no walk
    mat8, (qd, qo), (rd, ro) = ssw_wrap._pairs_inputs('test', refs, queries, match, mismatch, matrix, alphabet)
    rows, cig = _ctx().ends_batch(qd, qo, rd, ro, mat8, costs[0], costs[1], mode=mode, want_cigar=False, gap_open2=costs[2], gap_extend2=costs[3])
    assert len(cig) == 0
    for k, want in enumerate(wants):
        assert (int(rows[k]['score']), int(rows[k]['ref_end']), int(rows[k]['query_end'])) == (want['score'], want['ref_end'], want['query_end']), (k, mode, costs)
    return wants


@pytest.mark.parametrize('mode', MODES)
def test_geometry_around_the_lane_the_chunk_and_the_row_reload(mode):
    """n around a lane's 8 columns and one and two chunk borders (512, 1024), m around the 64-row reload: the third hand-over value
    crosses one and two borders"""
    rng = chk.rng_for('gpu twopiece grid', mode)
    refs, queries = [], []
    for n in (1, 7, 8, 9, 511, 512, 513, 1025):
        for m in (1, 63, 64, 65, 129):
            rs = chk.random_seq(rng, n)
            a = rng.randint(0, max(0, n - m))
            copy = chk.mutate(rng, rs[a:a + m], 0.08)
            refs.append(rs); queries.append((copy + chk.random_seq(rng, m))[:m])
    _check(refs, queries, mode, LONG)
    _check(refs[::3], queries[::3], mode, (3, 2, 6, 1))


def _planted(rng, n, L, at, kind):
    """a reference of n letters and a copy with 3 % substitutions, a 3-letter insertion near the start, and one planted gap of L
    letters: kind 'D' removes reference letters at[0] .. at[0] + L from the copy, 'I' adds L letters to the copy in front of at[0]"""
    ref = chk.random_seq(rng, n)
    q = list(ref)
    for x in range(n):
        if rng.random() < 0.03:
            q[x] = rng.choice([c for c in 'ACGT' if c != q[x]])
    a = at
    if kind == 'D':
        q = q[:a] + q[a + L:]
    else:
        q = q[:a] + list(chk.random_seq(rng, L)) + q[a:]
    q = q[:12] + list('TGA') + q[12:]
    return ref, ''.join(q)


@pytest.mark.parametrize('L', [20, 21, 22, 23, 40])
def test_crossover_a_planted_gap_is_paid_by_the_cheaper_piece(L):
    """a deletion, then an insertion, of L letters placed mid-lane, across a lane edge (column 8 k), across column 512 and at / across
    row 64: from 22 letters on only the two-piece programme gets the score, below that it is piece 1's"""
    # seeds at which the checker alone shows the premise below: among random letters a gap can also be split around chance matches
    rng = chk.rng_for('gpu twopiece crossover', L, {22: 5, 23: 14}.get(L, 0))
    refs, queries = [], []
    for n, at, kind in ((160, 83, 'D'), (200, 96 - L // 2, 'D'), (600, 512 - L // 2, 'D'), (300, 61, 'D'),
                        (160, 83, 'I'), (200, 96, 'I'), (600, 509, 'I'), (300, 64 - 3 - L // 2, 'I')):
        rs, qs = _planted(rng, n, L, at, kind)
        refs.append(rs); queries.append(qs)
    mat = chk.dna_matrix(2, 4)
    wants = []
    for rs, qs in zip(refs, queries):
        q, r = chk.encode(qs), chk.encode(rs)
        two = chk.align(q, r, mat, LONG, 'global')
        p1 = ec.align(q, r, mat, 4, 2, 'global', path=False)['score']
        p2 = ec.align(q, r, mat, 24, 1, 'global', path=False)['score']
        if L >= 22:
            assert two['score'] > p1 and two['score'] > p2, (L, two['score'], p1, p2)
            assert any(k == L for _, k in two['cigar']), two['cigar']
        else:
            assert two['score'] == p1 and two['score'] > p2, (L, two['score'], p1, p2)
        wants.append(two)
    _check(refs, queries, 'global', LONG, wants=wants)
    for mode in ('semiglobal', 'extend'):
        _check(refs, queries, mode, LONG)


@pytest.mark.parametrize('costs', [(3, 1, 3, 1), (3, 1, 8, 1), (4, 2, 4, 2), (4, 2, 9, 2)])
def test_a_dominated_second_piece_returns_the_one_piece_plan_s_rows_and_cigars(costs):
    from ciri_long_amd import hip
    rng = chk.rng_for('gpu twopiece dominated', costs)
    refs = [chk.random_seq(rng, n) for n in (5, 64, 200, 513, 700, 33)]
    queries = [chk.mutate(rng, r[rng.randint(0, len(r) // 3):], 0.15) or 'A' for r in refs]
    qd, qo = hip.pack(queries); rd, ro = hip.pack(refs)
    mat = hip.score_matrix(2, 4)
    for mode in MODES:
        one = _hip_rows(*_ctx().ends_batch(qd, qo, rd, ro, mat, costs[0], costs[1], mode=mode))
        two = _hip_rows(*_ctx().ends_batch(qd, qo, rd, ro, mat, costs[0], costs[1], mode=mode, gap_open2=costs[2], gap_extend2=costs[3]))
        assert one == two, mode


@pytest.mark.parametrize('costs', [(2, 2, 2, 2), (3, 3, 3, 3), (0, 0, 0, 0), (3, 2, 6, 1), (2, 1, 3, 0)])
def test_ties_equal_pieces_and_zero_costs(costs):
    rng = chk.rng_for('gpu twopiece ties', costs)
    refs, queries = [], []
    for t in range(16):
        alpha = 'AC' if t & 1 else 'ACGT'
        r = chk.random_seq(rng, rng.choice([6, 17, 40, 90, 530]), alpha)
        refs.append(r); queries.append(chk.mutate(rng, r, 0.4, alpha)[:200] or 'A')
    for mode in MODES:
        _check(refs, queries, mode, costs, match=1, mismatch=1)


@pytest.mark.parametrize('mode', ['global', 'semiglobal', 'extend'])
def test_blosum62_with_a_second_piece_that_extends_for_free(mode):
    from ciri_long_amd import ssw_wrap
    rng = chk.rng_for('gpu twopiece blosum', mode)
    letters = ssw_wrap.BLOSUM62_ALPHABET[:20]
    refs, queries = [], []
    for k in range(10):
        r = chk.random_seq(rng, rng.randint(60, 260), letters)
        a = rng.randint(20, len(r) - 35)
        q = chk.mutate(rng, r[:a] + r[a + 25:], 0.2, letters) if k & 1 else chk.random_seq(rng, rng.randint(50, 200), letters)
        refs.append(r); queries.append(q)
    _check(refs, queries, mode, (11, 1, 30, 0), matrix=ssw_wrap.BLOSUM62, alphabet=ssw_wrap.BLOSUM62_ALPHABET)


def test_empty_sides_are_the_boundary_under_the_cheaper_piece():
    refs = ['', 'ACGT' * 10, '', 'ACGTACGT']
    queries = ['ACGT' * 10, '', '', 'ACGTACGT']
    for mode in MODES:
        wants = _check(refs, queries, mode, LONG)
        if mode == 'global':
            assert wants[0]['score'] == wants[1]['score'] == -(24 + 39)          # 40 letters: piece 2, not 4 + 39 * 2
            assert wants[0]['cigar'] == [('I', 40)] and wants[1]['cigar'] == [('D', 40)]


def test_capacity_a_byte_per_cell_shares_in_both_orders_and_the_refusal():
    from ciri_long_amd import hip
    rng = chk.rng_for('gpu twopiece capacity')
    refs = [chk.random_seq(rng, n) for n in (600, 90, 300, 600, 40)]
    queries = [chk.mutate(rng, r[10:], 0.1) for r in refs]
    mat = hip.score_matrix(2, 4)
    cmat = chk.dna_matrix(2, 4)
    ctx = _ctx()
    for order in (1, -1):
        rs, qs = refs[::order], queries[::order]
        qd, qo = hip.pack(qs); rd, ro = hip.pack(rs)
        want = [chk.as_tuple(chk.align(chk.encode(q), chk.encode(r), cmat, LONG, 'global')) for q, r in zip(qs, rs)]
        one = ctx.ends_plan(qd, qo, rd, ro, mat, 4, 2)
        two = ctx.ends_plan(qd, qo, rd, ro, mat, 4, 2, gap_open2=24, gap_extend2=1)
        try:
            i1, i2 = one.info(), two.info()
            assert 2 * i1['max_pair_bytes'] - 16 <= i2['max_pair_bytes'] <= 2 * i1['max_pair_bytes']      # a byte per cell for half a byte, rounded up to 16
            assert 2 * i1['workspace_bytes'] - 16 * len(rs) <= i2['workspace_bytes'] <= 2 * i1['workspace_bytes']      # each pair's share is rounded up to 16
            assert i1['shares'] == i2['shares'] == 1
            two.run()
            assert _hip_rows(*two.fetch()) == want
        finally:
            one.close(); two.close()
        # what holds the largest pair of a one-piece plan does not hold it with two pieces
        assert ctx.ends_plan(qd, qo, rd, ro, mat, 4, 2, workspace_bytes=i1['max_pair_bytes']).close() is None
        with pytest.raises(hip.ClhError, match=r'alone needs \d+ bytes of workspace .* workspace_bytes is %d' % i1['max_pair_bytes']):
            ctx.ends_plan(qd, qo, rd, ro, mat, 4, 2, workspace_bytes=i1['max_pair_bytes'], gap_open2=24, gap_extend2=1)
        cut = ctx.ends_plan(qd, qo, rd, ro, mat, 4, 2, workspace_bytes=i2['max_pair_bytes'], gap_open2=24, gap_extend2=1)
        try:
            info = cut.info()
            assert info['shares'] >= 3 and info['workspace_bytes'] == i2['max_pair_bytes']
            cut.run()
            assert _hip_rows(*cut.fetch()) == want
            cut.run()
            assert _hip_rows(*cut.fetch()) == want
        finally:
            cut.close()


def test_costs_one_below_the_range_bound_and_the_refusal_at_it():
    from ciri_long_amd import hip, ssw_wrap
    big = 1 << 27                        # (4 + 4) 2^27 = 2^30 is the bound itself; the greatest cost is gap_open2
    kw = dict(match=2, mismatch=4, gap_open=4, gap_extend=2, gap_extend2=1)
    with pytest.raises(hip.ClhError, match=r'pair 1: \(m \+ n\) \* max\(\|s\|, gap_open, gap_extend, gap_open2, gap_extend2\) = 8 \* %d reaches 2\^30' % big):
        ssw_wrap.align_pairs_ends(['A', 'ACGT'], ['A', 'ACGT'], gap_open2=big, **kw)
    refs, queries = ['A', 'ACGT', 'ACGT'], ['A', 'ACGT', 'TTTT']
    for mode in MODES:
        _check(refs[:2], queries[:2], mode, (4, 2, big - 1, 1))
    # every cost just below the bound: the scores themselves come near -2^30
    c = big - 1
    for mode in MODES:
        _check(refs, queries, mode, (c, c, c, c), match=1, mismatch=1)
        _check(refs, queries, mode, (c, 0, c, 0), match=1, mismatch=1)


def test_refusals_name_the_violated_inequality():
    from ciri_long_amd import hip, ssw_wrap
    for costs, text in (((3, 2, 6, -1), r'0 <= gap_extend2'), ((3, 2, 6, 3), r'gap_extend2 <= gap_extend'), ((3, 2, 2, 1), r'gap_open <= gap_open2'),
                        ((1, 2, 6, 1), r'gap_open < gap_extend')):
        assert chk.violated(costs) is not None
        with pytest.raises(hip.ClhError, match=text):
            ssw_wrap.align_pairs_ends(['ACGT'], ['ACGT'], gap_open=costs[0], gap_extend=costs[1], gap_open2=costs[2], gap_extend2=costs[3])
    with pytest.raises(ValueError, match='come together'):
        _ctx().ends_plan(hip.encode('A'), [0, 1], hip.encode('A'), [0, 1], hip.score_matrix(2, 4), 4, 2, gap_open2=24)


def test_extend_anchors_with_the_long_read_preset_equals_the_checker_s_two_halves():
    from ciri_long_amd import ssw_wrap
    import anchored_check as ac
    rng = chk.rng_for('gpu twopiece anchors')
    p = ssw_wrap.LONG_READ_GAPS
    scoring = (p['match'], p['mismatch'], p['gap_open'], p['gap_extend'], p['gap_open2'], p['gap_extend2'])
    refs, queries, anchors = [], [], []
    for t in range(3):
        seed = chk.random_seq(rng, 20)
        left = chk.random_seq(rng, 150 + 40 * t); right = chk.random_seq(rng, 260)
        lq = chk.mutate(rng, left[:60] + left[60 + 30:], 0.04)                   # the query misses 30 letters on the left of the seed
        rq = chk.mutate(rng, right[:100] + chk.random_seq(rng, 35) + right[100:], 0.04)      # and carries 35 more on its right
        refs.append(left + seed + right); queries.append(lq + seed + rq)
        anchors.append((len(left), len(lq)))
    got = ssw_wrap.extend_anchors(refs, queries, anchors, seed_len=20, report_cigar=True, **p)
    long_runs = 0
    for k in range(3):
        want, _ = chk.expected_anchor(refs[k], queries[k], anchors[k], 20, scoring)
        g = got[k]
        assert (g.score, g.ref_begin, g.ref_end, g.query_begin, g.query_end, g.cigar_string) == want[:5] + (ac.text_of(want, len(queries[k])),), k
        long_runs += sum(1 for o, n in chk.parse_cigar(want[5]) if o in 'ID' and n >= 22)
    assert long_runs >= 3                # the planted events are kept as single long gaps, which piece 1 alone would not pay for


def test_cigars_with_as_many_runs_as_the_host_reserves():
    """the walk over bytes writes its last run at nops == cig_cap - 1: the one-piece checker's rows at (1, 0, 1, 0)"""
    import ends_edges as E
    from ciri_long_amd import ssw_wrap
    refs, queries, _ = E.max_runs_rows(E.HOST_GEOM)
    ma, mi, go, ge = E.MAX_RUNS_SCORING
    got = ssw_wrap.align_pairs_ends(refs, queries, mode='global', match=ma, mismatch=mi, gap_open=go, gap_extend=ge, gap_open2=go, gap_extend2=ge,
                                    report_cigar=True)
    E.check_max_runs(got, E.HOST_GEOM)


# ---- over a band (K1gb, csrc/ssw_band.hip) -------------------------------------------------------------------------------------------
BAND_MODES = chk.BAND_MODES


def _check_band(refs, queries, w, mode, costs, diagonals=None, match=2, mismatch=4, full_rows=None):
    """align_pairs_band with two pieces against the banded checker, field by field with band and exact, storing route and score-only
    route; with `full_rows` (the two-piece K1g rows of the same pairs on the same device) every certified row equals them"""
    from ciri_long_amd import hip, ssw_wrap
    mat = chk.dna_matrix(match, mismatch)
    kw = dict(mode=mode, diagonals=diagonals, match=match, mismatch=mismatch, gap_open=costs[0], gap_extend=costs[1], gap_open2=costs[2],
              gap_extend2=costs[3])
    got = ssw_wrap.align_pairs_band(refs, queries, w, report_cigar=True, **kw)
    wants = []
    for k, (rs, qs, g) in enumerate(zip(refs, queries, got)):
        q, r = chk.encode(qs), chk.encode(rs)
        lo, hi = chk.band_of(mode, len(q), len(r), w, None if diagonals is None else diagonals[k])
        want = chk.align_band(q, r, mat, costs, mode, lo, hi)
        have = (g.score, g.ref_begin, g.ref_end, g.query_begin, g.query_end, g.cigar_string, g.band, g.band_exact)
        assert have == chk.as_tuple(want)[:5] + (_text(want, len(qs)), (lo, hi), bool(want['exact'])), (k, mode, costs, w, len(qs), len(rs))
        ops = [(o, n) for o, n in chk.parse_cigar(g.cigar_string) if o != 'S']
        chk.check_cigar(dict(score=g.score, ref_begin=g.ref_begin, ref_end=g.ref_end, query_begin=g.query_begin, query_end=g.query_end, cigar=ops,
                             band=(lo, hi)), q, r, mat, costs, mode)
        if full_rows is not None and g.band_exact:
            f = full_rows[k]
            assert have[:6] == (f.score, f.ref_begin, f.ref_end, f.query_begin, f.query_end, f.cigar_string), (k, mode, 'certified row differs from K1g')
        wants.append(want)
    mat8, (qd, qo), (rd, ro) = ssw_wrap._pairs_inputs('test', refs, queries, match, mismatch, None, None)
    rows, cig = _ctx().band_batch(qd, qo, rd, ro, mat8, costs[0], costs[1], w, mode=mode, diagonals=diagonals, want_cigar=False,
                                  gap_open2=costs[2], gap_extend2=costs[3])
    assert len(cig) == 0
    for k, want in enumerate(wants):
        assert (int(rows[k]['score']), int(rows[k]['ref_end']), int(rows[k]['query_end']), int(rows[k]['exact'])) == \
            (want['score'], want['ref_end'], want['query_end'], want['exact']), (k, mode, costs, w)
    return wants


def _full(refs, queries, mode, costs, match=2, mismatch=4):
    from ciri_long_amd import ssw_wrap
    return ssw_wrap.align_pairs_ends(refs, queries, mode=mode, match=match, mismatch=mismatch, gap_open=costs[0], gap_extend=costs[1], gap_open2=costs[2],
                                     gap_extend2=costs[3], report_cigar=True)


def test_band_cigars_with_as_many_runs_as_the_host_reserves():
    """as above over a band that clips to the whole matrix (the widest pair spans 156 diagonals)"""
    import ends_edges as E
    from ciri_long_amd import ssw_wrap
    refs, queries, _ = E.max_runs_rows(E.HOST_GEOM)
    ma, mi, go, ge = E.MAX_RUNS_SCORING
    got = ssw_wrap.align_pairs_band(refs, queries, 128, mode='global', match=ma, mismatch=mi, gap_open=go, gap_extend=ge, gap_open2=go, gap_extend2=ge,
                                    report_cigar=True)
    E.check_max_runs(got, E.HOST_GEOM)
    assert all(g.band_exact for g in got)


WIDTHS = [(1, 0, 0), (2, 0, 1), (127, 63, 0), (128, 63, 1), (129, 64, 0), (255, 127, 0), (256, 127, 1), (257, 128, 0), (511, 255, 0), (512, 255, 1)]


@pytest.mark.parametrize('width,w,dn', WIDTHS, ids=[str(x[0]) for x in WIDTHS])
def test_band_clipped_widths_around_the_class_edges(width, w, dn):
    """widths at the edges of the classes of 2, 4 and 8 positions per lane (128, 256, 512 diagonals)"""
    rng = chk.rng_for('gpu twopiece widths', width)
    m = 300
    rs = [chk.random_seq(rng, m + dn), chk.random_seq(rng, m + dn)]
    qs = [(chk.mutate(rng, rs[0], 0.1) + chk.random_seq(rng, m))[:m], chk.random_seq(rng, m)]
    for mode in ('global', 'semiglobal'):          # [min(0, n - m) - w, max(0, n - m) + w]
        wants = _check_band(rs, qs, w, mode, LONG, full_rows=_full(rs, qs, mode, LONG))
        assert all(x['band'][1] - x['band'][0] + 1 == width for x in wants)
    if width > 2:                                  # start-anchored: [-w, w], an even width by clipping lo at -m = -(w - 1)
        w2 = width // 2
        qs2 = qs if width % 2 else [q[:w2 - 1] for q in qs]
        for mode in ('prefix', 'extend'):
            wants = _check_band(rs, qs2, w2, mode, LONG, full_rows=_full(rs, qs2, mode, LONG))
            assert all(x['band'][1] - x['band'][0] + 1 == width for x in wants)


@pytest.mark.parametrize('mode', BAND_MODES)
def test_band_rows_around_the_64_row_reload(mode):
    rng = chk.rng_for('gpu twopiece band rows', mode)
    refs, queries = [], []
    for m in (1, 63, 64, 65, 129):
        rs = chk.random_seq(rng, m + 7)
        refs.append(rs); queries.append((chk.mutate(rng, rs[3:], 0.1) + chk.random_seq(rng, m))[:m])
    for w in (5, 140):
        _check_band(refs, queries, w, mode, LONG, full_rows=_full(refs, queries, mode, LONG))
    _check_band(refs, queries, 9, mode, (3, 2, 6, 1))


@pytest.mark.parametrize('w', [12, 30])
def test_band_a_planted_gap_of_the_half_width_and_one_more_in_both_pieces_ranges(w):
    """a deletion and an insertion of exactly w letters stay in the band, of w + 1 leave it; w = 12 is paid by piece 1, w = 30 by
    piece 2 (the pieces swap at 22); every certified row equals the two-piece K1g row"""
    rng = chk.rng_for('gpu twopiece half-width', w)
    refs, queries = [], []
    for L in (w, w + 1):
        for kind in ('D', 'I'):
            rs, qs = _planted(rng, 300, L, 140, kind)
            rs, qs = rs[20:], qs[23:]                          # without the 3-letter insertion of _planted: the gap alone moves the diagonal
            tail = chk.random_seq(rng, L)                      # and both ends back on diagonal 0, so that global's corner is in the band
            if kind == 'D':
                qs += tail
            else:
                rs += tail
            refs.append(rs); queries.append(qs)
    for mode in BAND_MODES:
        wants = _check_band(refs, queries, w, mode, LONG, full_rows=_full(refs, queries, mode, LONG))
        if mode == 'extend':
            assert any(k == w for o, k in wants[0]['cigar'] if o == 'D') and any(k == w for o, k in wants[1]['cigar'] if o == 'I')
            assert not any(k > w for o, k in wants[2]['cigar'] + wants[3]['cigar'] if o in 'ID')


def test_band_hints_place_semiglobal_queries_and_certified_rows_equal_k1g():
    rng = chk.rng_for('gpu twopiece hints')
    refs, queries, diags = [], [], []
    for t in range(12):
        rs = chk.random_seq(rng, rng.choice([200, 513, 700]))
        a = rng.randint(0, len(rs) - 120)
        piece = rs[a:a + 120]
        qs = chk.mutate(rng, piece[:50] + piece[50 + (25 if t % 3 == 0 else 4):], 0.05)
        refs.append(rs); queries.append(qs); diags.append(a + rng.randint(-3, 3))
    _check_band(refs, queries, 40, 'semiglobal', LONG, diagonals=diags)
    for mode in ('global', 'prefix', 'extend'):
        rs2 = [r[d:d + 150] if mode != 'global' else r[max(0, d):max(0, d) + len(q) + 10] for r, q, d in zip(refs, queries, diags)]
        for w in (3, 16, 45):
            _check_band(rs2, queries, w, mode, LONG, full_rows=_full(rs2, queries, mode, LONG))


@pytest.mark.parametrize('costs', [(3, 1, 3, 1), (4, 2, 9, 2)])
def test_band_a_dominated_second_piece_returns_the_one_piece_plan_s_rows(costs):
    from ciri_long_amd import hip
    rng = chk.rng_for('gpu twopiece band dominated', costs)
    refs = [chk.random_seq(rng, n) for n in (5, 64, 200, 513, 700, 33)]
    queries = [chk.mutate(rng, r, 0.15)[:len(r)] or 'A' for r in refs]          # m <= n: prefix has its end cell at every width
    qd, qo = hip.pack(queries); rd, ro = hip.pack(refs)
    mat = hip.score_matrix(2, 4)
    for mode in BAND_MODES:
        for w in (10, 100, 200):
            one = _ctx().band_batch(qd, qo, rd, ro, mat, costs[0], costs[1], w, mode=mode)
            two = _ctx().band_batch(qd, qo, rd, ro, mat, costs[0], costs[1], w, mode=mode, gap_open2=costs[2], gap_extend2=costs[3])
            assert _hip_rows(*one) == _hip_rows(*two), (mode, w)
            full = _hip_rows(*_ctx().ends_batch(qd, qo, rd, ro, mat, costs[0], costs[1], mode=mode, gap_open2=costs[2], gap_extend2=costs[3]))
            assert all(a == b for a, b, x in zip(_hip_rows(*two), full, two[0]['exact']) if x), (mode, w)       # certified rows are K1g's
            assert (one[0]['exact'] == two[0]['exact']).all() and (one[0]['band_lo'] == two[0]['band_lo']).all()


@pytest.mark.parametrize('costs', [(2, 2, 2, 2), (0, 0, 0, 0), (3, 2, 6, 1), (2, 1, 3, 0)])
def test_band_ties_equal_pieces_and_zero_costs(costs):
    rng = chk.rng_for('gpu twopiece band ties', costs)
    refs, queries = [], []
    for t in range(12):
        alpha = 'AC' if t & 1 else 'ACGT'
        r = chk.random_seq(rng, rng.choice([6, 17, 40, 90, 300]), alpha)
        refs.append(r); queries.append(chk.mutate(rng, r, 0.3, alpha)[:len(r)] or 'A')      # m <= n: prefix has its end cell at every width
    for mode in BAND_MODES:
        for w in (4, 70):
            _check_band(refs, queries, w, mode, costs, match=1, mismatch=1, full_rows=_full(refs, queries, mode, costs, match=1, mismatch=1))


def test_band_capacity_a_byte_per_cell_shares_and_the_range_bound():
    from ciri_long_amd import hip, ssw_wrap
    rng = chk.rng_for('gpu twopiece band capacity')
    refs = [chk.random_seq(rng, n) for n in (600, 90, 300, 600, 40)]
    queries = [chk.mutate(rng, r, 0.1) for r in refs]
    mat = hip.score_matrix(2, 4)
    cmat = chk.dna_matrix(2, 4)
    ctx = _ctx()
    for order in (1, -1):
        rs, qs = refs[::order], queries[::order]
        qd, qo = hip.pack(qs); rd, ro = hip.pack(rs)
        want = []
        for q, r in zip(qs, rs):
            lo, hi = chk.band_of('global', len(q), len(r), 20)
            want.append(chk.as_tuple(chk.align_band(chk.encode(q), chk.encode(r), cmat, LONG, 'global', lo, hi)))
        one = ctx.band_plan(qd, qo, rd, ro, mat, 4, 2, 20)
        two = ctx.band_plan(qd, qo, rd, ro, mat, 4, 2, 20, gap_open2=24, gap_extend2=1)
        try:
            i1, i2 = one.info(), two.info()
            assert 2 * i1['max_pair_bytes'] - 16 <= i2['max_pair_bytes'] <= 2 * i1['max_pair_bytes'] and i1['shares'] == i2['shares'] == 1
            two.run()
            assert _hip_rows(*two.fetch()) == want
        finally:
            one.close(); two.close()
        assert ctx.band_plan(qd, qo, rd, ro, mat, 4, 2, 20, workspace_bytes=i1['max_pair_bytes']).close() is None
        with pytest.raises(hip.ClhError, match=r'alone needs \d+ bytes of workspace .* workspace_bytes is %d' % i1['max_pair_bytes']):
            ctx.band_plan(qd, qo, rd, ro, mat, 4, 2, 20, workspace_bytes=i1['max_pair_bytes'], gap_open2=24, gap_extend2=1)
        cut = ctx.band_plan(qd, qo, rd, ro, mat, 4, 2, 20, workspace_bytes=i2['max_pair_bytes'], gap_open2=24, gap_extend2=1)
        try:
            assert cut.info()['shares'] >= 3 and cut.info()['workspace_bytes'] == i2['max_pair_bytes']
            cut.run()
            assert _hip_rows(*cut.fetch()) == want
        finally:
            cut.close()
    big = (1 << 29) // (4 + 4 + 1024)          # (m + n + 1024) * big reaches 2^29 at the first value above this
    kw = dict(match=2, mismatch=4, gap_open=4, gap_extend=2, gap_extend2=1)
    with pytest.raises(hip.ClhError, match=r'gap_open, gap_extend, gap_open2, gap_extend2\) = 1032 \* %d reaches 2\^29' % (big + 1)):
        ssw_wrap.align_pairs_band(['ACGT'], ['ACGT'], 2, gap_open2=big + 1, **kw)
    for mode in BAND_MODES:
        _check_band(['ACGT', 'ACGT'], ['ACGT', 'TTTT'], 2, mode, (4, 2, big, 1))
    with pytest.raises(hip.ClhError, match=r'gap_open <= gap_open2'):
        ssw_wrap.align_pairs_band(['ACGT'], ['ACGT'], 2, gap_open=4, gap_extend=2, gap_open2=3, gap_extend2=1)
    with pytest.raises(hip.ClhError, match=r'gap_extend2 <= gap_extend'):
        ssw_wrap.align_pairs_band(['ACGT'], ['ACGT'], 2, gap_open=4, gap_extend=2, gap_open2=24, gap_extend2=3)


def test_extend_anchors_under_a_band_of_64_with_the_long_read_preset():
    from ciri_long_amd import ssw_wrap
    import anchored_check as ac
    rng = chk.rng_for('gpu twopiece anchors')              # the pairs of the unbanded test
    p = ssw_wrap.LONG_READ_GAPS
    scoring = (p['match'], p['mismatch'], p['gap_open'], p['gap_extend'], p['gap_open2'], p['gap_extend2'])
    refs, queries, anchors = [], [], []
    for t in range(3):
        seed = chk.random_seq(rng, 20)
        left = chk.random_seq(rng, 150 + 40 * t); right = chk.random_seq(rng, 260)
        lq = chk.mutate(rng, left[:60] + left[60 + 30:], 0.04)
        rq = chk.mutate(rng, right[:100] + chk.random_seq(rng, 35) + right[100:], 0.04)
        refs.append(left + seed + right); queries.append(lq + seed + rq)
        anchors.append((len(left), len(lq)))
    got = ssw_wrap.extend_anchors(refs, queries, anchors, band=64, seed_len=20, report_cigar=True, **p)
    for k in range(3):
        want, exact = chk.expected_anchor(refs[k], queries[k], anchors[k], 20, scoring, band=64)
        g = got[k]
        assert (g.score, g.ref_begin, g.ref_end, g.query_begin, g.query_end, g.cigar_string, g.band_exact) == \
            want[:5] + (ac.text_of(want, len(queries[k])), bool(exact)), k


def test_the_batch_calls_of_the_c_abi_with_a_second_piece_and_with_none():
    """clh_ends_batch_gap2 and clh_band_batch_gap2 called as C callers do: with a clh_gap2 they return the two-piece plan's rows, with a
    null gap2 the one-piece call's"""
    import ctypes as C
    from ciri_long_amd import hip
    rng = chk.rng_for('gpu twopiece batch abi')
    refs = [chk.random_seq(rng, n) for n in (40, 300, 600)]
    queries = [chk.mutate(rng, r[:25] + r[25 + 30:], 0.05) for r in refs]        # 30 letters missing: piece 2 pays
    qd, qo = hip.pack(queries); rd, ro = hip.pack(refs)
    qd = np.ascontiguousarray(qd, dtype=np.int8); rd = np.ascontiguousarray(rd, dtype=np.int8)
    qo = np.ascontiguousarray(qo, dtype=np.int64); ro = np.ascontiguousarray(ro, dtype=np.int64)
    mat = np.ascontiguousarray(hip.score_matrix(2, 4), dtype=np.int8).reshape(-1)
    ctx = _ctx()
    L = hip.lib()
    n = len(refs)
    cap = int(sum(len(q) + len(r) for q, r in zip(queries, refs)))
    gap2 = hip.Gap2(24, 1)

    def call(kind, with_gap2):
        rows = np.zeros(n, dtype=hip.ENDS_DTYPE if kind == 'ends' else hip.BAND_DTYPE)
        cig = np.zeros(cap, dtype=np.uint32)
        used = C.c_int64(0)
        g = C.byref(gap2) if with_gap2 else None
        if kind == 'ends':
            opts = hip.EndsOpts(hip.ENDS_MODES['global'], mat.ctypes.data, 5, 4, 2, 1, 0)
            rc = L.clh_ends_batch_gap2(ctx._h, n, qd.ctypes.data, qo.ctypes.data, rd.ctypes.data, ro.ctypes.data, C.byref(opts), g,
                                       rows.ctypes.data, cig.ctypes.data, cap, C.byref(used))
        else:
            opts = hip.BandOpts(hip.ENDS_MODES['global'], mat.ctypes.data, 5, 4, 2, 1, 0, 40, 0)
            rc = L.clh_band_batch_gap2(ctx._h, n, qd.ctypes.data, qo.ctypes.data, rd.ctypes.data, ro.ctypes.data, None, C.byref(opts), g,
                                       rows.ctypes.data, cig.ctypes.data, cap, C.byref(used))
        assert rc == 0, hip.last_error()
        return _hip_rows(rows, cig[:used.value]), rows
    cmat = chk.dna_matrix(2, 4)
    enc = [(chk.encode(q), chk.encode(r)) for q, r in zip(queries, refs)]
    got, _ = call('ends', True)
    assert got == [chk.as_tuple(chk.align(q, r, cmat, LONG, 'global')) for q, r in enc]
    assert any('30D' in g[5] for g in got)
    got, _ = call('ends', False)
    assert got == _hip_rows(*ctx.ends_batch(qd, qo, rd, ro, mat, 4, 2)) == [ec.as_tuple(ec.align(q, r, cmat, 4, 2, 'global')) for q, r in enc]
    got, rows = call('band', True)
    wants = [chk.align_band(q, r, cmat, LONG, 'global', *chk.band_of('global', len(q), len(r), 40)) for q, r in enc]
    assert got == [chk.as_tuple(w) for w in wants] and [int(x) for x in rows['exact']] == [w['exact'] for w in wants]
    got, rows = call('band', False)
    one = ctx.band_batch(qd, qo, rd, ro, mat, 4, 2, 40)
    assert got == _hip_rows(*one) and (rows['exact'] == one[0]['exact']).all()
