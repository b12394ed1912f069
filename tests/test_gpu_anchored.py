"""Start-anchored alignment of pairs on the GPU: modes prefix and extend of K1g (csrc/ssw_ends.hip) and K1gb (csrc/ssw_band.hip),
and ssw_wrap.extend_anchors.  Every expected value is tests/anchored_check.py, field by field with CIGARs; shapes are the smallest
at which the kernels can go wrong (lane, register, chunk, class and share edges come from the plans' own geometry)."""
import numpy as np
import pytest

import anchored_check as chk

pytestmark = pytest.mark.gpu

MODES = chk.MODES
SCORINGS = [(2, 2, 3, 1), (10, 4, 8, 2)]
OPS = 'MID'


def _ctx():
    from ciri_long_amd import hip
    return hip.default_context()


@pytest.fixture(scope='module')
def geom():
    from ciri_long_amd import hip
    plan = _ctx().ends_plan(hip.encode('A'), [0, 1], hip.encode('A'), [0, 1], hip.score_matrix(2, 2), 3, 1, mode='extend')
    try:
        g = plan.info()
    finally:
        plan.close()
    assert g['cpl'] >= 1 and g['chunk'] == 64 * g['cpl']
    return g


def _rows(qs, rs, mat, go, ge, mode, band=None, diagonals=None, want_cigar=True, workspace_bytes=0, info=None):
    """Context.ends_plan (band None) or band_plan on sequences of codes -> one tuple per pair as ends_check.as_tuple writes it, plus
    (band, exact) under a band"""
    from ciri_long_amd import hip
    qd, qo = hip.pack([np.asarray(q, dtype=np.int8) for q in qs]); rd, ro = hip.pack([np.asarray(r, dtype=np.int8) for r in rs])
    flat = np.asarray(mat, dtype=np.int8).reshape(-1)                   # row = reference code, as the checker's
    if band is None:
        plan = _ctx().ends_plan(qd, qo, rd, ro, flat, go, ge, mode=mode, want_cigar=want_cigar, workspace_bytes=workspace_bytes)
    else:
        plan = _ctx().band_plan(qd, qo, rd, ro, flat, go, ge, band, mode=mode, diagonals=diagonals, want_cigar=want_cigar, workspace_bytes=workspace_bytes)
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
        t = (int(r['score']), int(r['ref_begin']), int(r['ref_end']), int(r['query_begin']), int(r['query_end']), ops)
        out.append(t if band is None else t + ((int(r['band_lo']), int(r['band_hi'])), int(r['exact'])))
    return out


def _check(qs, rs, mat, go, ge, mode, band=None, diagonals=None, **kw):
    """the storing and the score-only route against the checker -> the checker's results"""
    qs = [np.asarray(q, dtype=np.int64) for q in qs]; rs = [np.asarray(r, dtype=np.int64) for r in rs]
    wants = []
    for k, (q, r) in enumerate(zip(qs, rs)):
        if band is None:
            wants.append(chk.align(q, r, mat, go, ge, mode))
        else:
            lo, hi = chk.band_of(len(q), len(r), band, None if diagonals is None else diagonals[k])
            wants.append(chk.align_band(q, r, mat, go, ge, mode, lo, hi))
    got = _rows(qs, rs, mat, go, ge, mode, band, diagonals, True, **kw)
    bare = _rows(qs, rs, mat, go, ge, mode, band, diagonals, False)
    for k, want in enumerate(wants):
        full = chk.as_tuple(want) + ((tuple(want['band']), want['exact']) if band is not None else ())
        assert got[k] == full, (k, mode, (go, ge), band, len(qs[k]), len(rs[k]))
        chk.check_cigar(want, qs[k], rs[k], mat, go, ge, mode)
        assert bare[k] == full[:5] + (None,) + full[6:], (k, mode)       # both begins are fixed by the mode: 0 without the walk too
    return wants


def _dna(strings):
    return [chk.encode(s) for s in strings]


def _flank(rng, rs, m, keep, rate=0.10):
    """a query of m letters: a mutated copy of rs[:keep], then unrelated letters"""
    return (chk.mutate(rng, rs[:keep], rate) + chk.random_seq(rng, m))[:m]


# ----------------------------------------------------------------------------------------------------------------------------
# K1g
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
def test_length_grid_around_the_lane_the_row_block_and_the_chunk(geom, mode):
    assert (geom['cpl'], geom['chunk']) == (8, 512)           # the lengths below are this geometry's edges
    rng = chk.rng_for('gpu anchored grid', mode)
    qs, rs = [], []
    for n in (1, 8, 9, 511, 512, 513, 1025):
        for m in (1, 63, 64, 65, 129):
            r = chk.random_seq(rng, n)
            rs.append(r); qs.append(chk.random_seq(rng, m))
            rs.append(r); qs.append(_flank(rng, r, m, rng.randint(1, n)))
    for ma, mi, go, ge in SCORINGS:
        _check(_dna(qs), _dna(rs), chk.dna_matrix(ma, mi), go, ge, mode)


def test_the_best_cell_in_every_register_of_a_lane_and_in_the_first_last_and_partial_lane(geom):
    cpl, C = geom['cpl'], geom['chunk']
    rng = chk.rng_for('gpu anchored planted')
    qs, rs, cols = [], [], []
    # (columns of the reference, the column j of the best cell): lane 0, lane 63, a lane inside, and the last lane of a reference
    # that ends inside it, each in every register; then the same lanes of the second chunk
    plant = [(C, j) for j in range(1, cpl + 1)] + [(C, C - cpl + k) for k in range(1, cpl + 1)] + \
            [(C, 20 * cpl + k) for k in range(1, cpl + 1)] + [(12 * cpl + 3, 12 * cpl + k) for k in (1, 2, 3)] + \
            [(2 * C, C + k) for k in (1, cpl)] + [(2 * C, 2 * C - k) for k in (0, cpl - 1)] + [(C + 2 * cpl + 3, C + 2 * cpl + k) for k in (1, 3)]
    for n, j in plant:
        core = chk.random_seq(rng, j, 'ACG')
        rs.append(core + 'T' * (n - j)); qs.append(core + 'A' * 5)       # nothing beyond (j, j) matches: the best cell is (j, j)
        cols.append(j)
    wants = _check(_dna(qs), _dna(rs), chk.dna_matrix(2, 2), 3, 1, 'extend')
    assert [(w['query_end'] + 1, w['ref_end'] + 1) for w in wants] == [(j, j) for j in cols]


def test_equal_scores_in_two_chunks_go_to_the_smaller_row_then_the_smaller_column(geom):
    C = geom['chunk']
    free = chk.dna_matrix(1, 0)             # free gaps, match 1, mismatch 0: H is the length of a common subsequence
    qs = ['CA', 'AC', 'GCA', 'CA']
    rs = ['A' + 'G' * (C - 1) + 'C',        # 1 at (1, C + 1), chunk 2, and at (2, 1), chunk 1, which the lanes meet first
          'A' + 'G' * (C + 40),             # the reverse: 1 at (1, 1), chunk 1, and again along rows 1 and 2 of chunk 2
          'A' + 'T' * (2 * C - 1) + 'C',    # 1 at (2, 2 C + 1), chunk 3, and at (3, 1), chunk 1
          'A' + 'G' * (C - 1) + 'C' + 'G' * C]
    wants = _check(_dna(qs), _dna(rs), free, 0, 0, 'extend')
    assert [(w['score'], w['query_end'] + 1, w['ref_end'] + 1) for w in wants] == [(1, 1, C + 1), (1, 1, 1), (1, 2, 2 * C + 1), (1, 1, C + 1)]
    _check(_dna(qs), _dna(rs), free, 0, 0, 'prefix')


def test_nothing_to_extend_gives_the_empty_result(geom):
    from ciri_long_amd import ssw_wrap
    C = geom['chunk']
    qs, rs = ['A' * 5, 'A' * 70, 'C', 'ACGT', ''], ['C' * 9, 'C' * (C + 3), 'A', '', 'ACGT']
    got = ssw_wrap.align_pairs_ends(rs, qs, mode='extend', report_cigar=True)
    for g, q in zip(got, qs):
        assert (g.score, g.ref_begin, g.ref_end, g.query_begin, g.query_end, g.cigar_string) == (0, 0, -1, 0, -1, '%dS' % len(q) if q else '')
    _check(_dna(qs[:3]), _dna(rs[:3]), chk.dna_matrix(2, 2), 3, 1, 'extend')
    got = ssw_wrap.align_pairs_ends(rs, qs, mode='prefix', report_cigar=True)          # the empty sides of prefix: mI, or nothing
    assert [(g.score, g.ref_end, g.query_end, g.cigar_string) for g in got[3:]] == [(-6, -1, 3, '4I'), (0, -1, -1, '')]


@pytest.mark.parametrize('mode', MODES)
def test_free_gaps_and_a_protein_matrix(geom, mode):
    from ciri_long_amd import ssw_wrap
    rng = chk.rng_for('gpu anchored free gaps', mode)
    rs = [chk.random_seq(rng, n, 'AC' if n & 1 else 'ACGT') for n in (5, 64, 65, geom['chunk'] + 9)]
    qs = [_flank(rng, r, m, len(r) // 2, 0.2) for r, m in zip(rs, (7, 40, 70, 66))]
    _check(_dna(qs), _dna(rs), chk.dna_matrix(2, 2), 0, 0, mode)
    _check(_dna(qs), _dna(rs), chk.dna_matrix(1, 3), 2, 0, mode)
    letters = ssw_wrap.BLOSUM62_ALPHABET[:20]
    prs = [chk.random_seq(rng, n, letters) for n in (30, 200)]
    pqs = [(chk.mutate(rng, r[:len(r) // 2], 0.2, letters) + chk.random_seq(rng, 20, letters)) for r in prs]
    mat = ssw_wrap.BLOSUM62.astype(np.int64)
    got = ssw_wrap.align_pairs_ends(prs, pqs, mode=mode, gap_open=11, gap_extend=1, report_cigar=True, matrix=ssw_wrap.BLOSUM62,
                                    alphabet=ssw_wrap.BLOSUM62_ALPHABET)
    for g, qs_, rs_ in zip(got, pqs, prs):
        want = chk.align(chk.encode(qs_, ssw_wrap.BLOSUM62_ALPHABET), chk.encode(rs_, ssw_wrap.BLOSUM62_ALPHABET), mat, 11, 1, mode)
        tail = len(qs_) - want['query_end'] - 1
        assert (g.score, g.ref_begin, g.ref_end, g.query_begin, g.query_end, g.cigar_string) == \
            chk.as_tuple(want)[:5] + (chk.cigar_text(want['cigar']) + ('%dS' % tail if tail else ''),)
    assert got[1].score > 100 or mode == 'prefix'


@pytest.mark.parametrize('mode', MODES)
def test_shares_at_a_workspace_of_exactly_the_largest_pair(geom, mode):
    from ciri_long_amd import hip
    rng = chk.rng_for('gpu anchored shares', mode)
    rs = [chk.random_seq(rng, n) for n in (100, geom['chunk'] + 5, 30, 100, 64)]
    qs = [_flank(rng, r, 60, 40) for r in rs]
    mat = chk.dna_matrix(2, 2)
    whole, cut = {}, {}
    a = _rows(_dna(qs), _dna(rs), mat, 3, 1, mode, info=whole)
    top = whole['max_pair_bytes']
    b = _rows(_dna(qs), _dna(rs), mat, 3, 1, mode, info=cut, workspace_bytes=top)
    assert whole['shares'] == 1 and cut['shares'] >= 3 and cut['workspace_bytes'] == top == cut['max_pair_bytes']
    assert a == b == [chk.as_tuple(chk.align(q, r, mat, 3, 1, mode)) for q, r in zip(_dna(qs), _dna(rs))]
    qd, qo = hip.pack([hip.encode(q) for q in qs]); rd, ro = hip.pack([hip.encode(r) for r in rs])
    with pytest.raises(hip.ClhError, match='workspace'):
        _ctx().ends_plan(qd, qo, rd, ro, hip.score_matrix(2, 2), 3, 1, mode=mode, workspace_bytes=top - 16)


def test_the_score_bound_one_below_and_at_two_to_the_thirty():
    from ciri_long_amd import hip, ssw_wrap
    for mode, scores in (('extend', [2, 8]), ('prefix', [2, 8])):
        with pytest.raises(hip.ClhError, match=r'pair 1: .*reaches 2\^30'):          # (4 + 4) 2^27 is the bound itself
            ssw_wrap.align_pairs_ends(['A', 'ACGT'], ['A', 'ACGT'], mode=mode, gap_open=1 << 27, gap_extend=0)
        ok = ssw_wrap.align_pairs_ends(['A', 'ACGT'], ['A', 'ACGT'], mode=mode, gap_open=(1 << 27) - 1, gap_extend=0, report_cigar=True)
        assert [g.score for g in ok] == scores and [g.cigar_string for g in ok] == ['1M', '4M']
    # a gap at the bound's cost is taken where nothing else is left: prefix of a query against an unrelated letter
    g, = ssw_wrap.align_pairs_ends(['C'], ['AAA'], mode='prefix', match=1, mismatch=1, gap_open=(1 << 28) - 1, gap_extend=0, report_cigar=True)
    want = chk.align(chk.encode('AAA'), chk.encode('C'), chk.dna_matrix(1, 1), (1 << 28) - 1, 0, 'prefix')
    assert (g.score, g.ref_end, g.query_end, g.cigar_string) == (want['score'], want['ref_end'], want['query_end'], chk.cigar_text(want['cigar']))


def test_prefix_at_unit_costs_is_edlib_shw_on_the_device():
    from ciri_long_amd import edlib, ssw_wrap
    rng = chk.rng_for('gpu anchored shw')
    ts = [chk.random_seq(rng, n, 'AC' if n & 1 else 'ACGT') for n in (1, 9, 40, 64, 65, 130, 600)] + ['CCCC', 'TTTT']
    qs = [(chk.mutate(rng, t[:max(1, len(t) // 2)], 0.15) or 'A') for t in ts[:-2]] + ['AAAA', 'ACGT']
    got = ssw_wrap.align_pairs_ends(ts, qs, mode='prefix', match=0, mismatch=1, gap_open=1, gap_extend=1)
    col0 = 0
    for q, t, g in zip(qs, ts, got):
        e = edlib.align(q, t, mode='SHW', task='locations')
        # edlib's SHW never ends at column 0; the programme here does where deleting the whole query (distance m) is as good
        want_end = -1 if e['editDistance'] == len(q) else e['locations'][0][1]
        assert (g.score, g.ref_end, g.ref_begin, g.query_begin, g.query_end) == (-e['editDistance'], want_end, 0, 0, len(q) - 1), (q, t)
        col0 += want_end == -1
    assert col0 >= 1


# ----------------------------------------------------------------------------------------------------------------------------
# K1gb
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def bgeom():
    from ciri_long_amd import hip
    plan = _ctx().band_plan(hip.encode('A'), [0, 1], hip.encode('A'), [0, 1], hip.score_matrix(2, 2), 3, 1, 0, mode='extend')
    try:
        g = plan.info()
    finally:
        plan.close()
    assert g['cpl'] == [2, 4, 8] and g['class_pairs'] == [1, 0, 0] and g['max_width'] == 1
    return g


# (clipped width, half-width, diagonal hint, short side): the band is [-w, w] around 0, or around the hint, 2 w + 1 wide; an even
# width comes from clipping at a short side of w - 1 letters -- the reference for extend, the query for prefix, whose band must
# reach row m -- and width 2 from the hint 1 over a reference of one letter
WIDTHS = [(1, 0, None, None), (2, 1, 1, 1), (127, 63, None, None), (128, 64, None, 63), (129, 64, None, None), (255, 127, None, None),
          (256, 128, None, 127), (257, 128, None, None), (511, 255, None, None), (512, 256, None, 255)]


@pytest.mark.parametrize('width,w,diag,short', WIDTHS, ids=[str(x[0]) for x in WIDTHS])
def test_clipped_widths_around_the_class_edges(bgeom, width, w, diag, short):
    rng = chk.rng_for('gpu anchored widths', width)
    long_ = 300
    for mode in MODES:
        if short is None:
            m, n = long_, long_ + 7
        elif diag is not None or mode == 'extend':
            m, n = long_, short
        else:
            m, n = short, long_
        if mode == 'prefix' and n - m < -w:
            m = n                                               # width 2: the band [0, 1] of the one-letter reference holds row m only for m <= 1
        rs = [chk.random_seq(rng, n), chk.random_seq(rng, n)]
        qs = [_flank(rng, rs[0], m, max(1, min(m, n) * 2 // 3)), chk.random_seq(rng, m)]
        info = {}
        wants = _check(_dna(qs), _dna(rs), chk.dna_matrix(2, 2), 3, 1, mode, band=w, diagonals=None if diag is None else [diag, diag], info=info)
        assert all(x['band'][1] - x['band'][0] + 1 == width for x in wants), (mode, [x['band'] for x in wants])
        assert info['max_width'] == width
        assert info['class_pairs'] == [2 if c == min(c2 for c2, cpl in enumerate(bgeom['cpl']) if width <= 64 * cpl) else 0 for c in range(3)]


def test_the_best_cell_on_the_bands_edges_and_on_the_first_and_last_row(bgeom):
    rng = chk.rng_for('gpu anchored band planted')
    w = 6
    core = chk.random_seq(rng, 40, 'ACG')
    qs = [core + 'A' * 4, 'G' * w + core + 'A' * 4, core[:1] + 'T' * 9, core]
    rs = ['G' * w + core + 'T' * 9, core + 'T' * 9, core[:1] + 'A' * 9, core + 'A' * 9]
    wants = _check(_dna(qs), _dna(rs), chk.dna_matrix(10, 9), 3, 0, 'extend', band=w)
    ends = [(x['query_end'] + 1, x['ref_end'] + 1) for x in wants]
    assert ends == [(40, 40 + w), (40 + w, 40), (1, 1), (40, 40)], ends          # diagonal hi, diagonal lo, row 1, row m
    assert [x['ref_end'] - x['query_end'] for x in wants[:2]] == [w, -w]
    _check(_dna(qs), _dna(rs), chk.dna_matrix(10, 9), 3, 0, 'prefix', band=w + 4)


def test_prefix_ends_at_column_0_inside_the_band(bgeom):
    wants = _check(_dna(['AAA', 'AAA']), _dna(['CCCCC', 'C']), chk.dna_matrix(1, 30), 2, 1, 'prefix', band=3)
    assert [(x['score'], x['ref_end'], chk.cigar_text(x['cigar'])) for x in wants] == [(-4, -1, '3I'), (-4, -1, '3I')]


def test_refusals_carry_their_messages(bgeom):
    from ciri_long_amd import hip, ssw_wrap
    ref, qry = 'ACGT' * 10, 'ACGT' * 5
    with pytest.raises(hip.ClhError, match=r'pair 1: the band \[3, 7\] of the 20 x 40 pair misses \(0, 0\)'):
        ssw_wrap.align_pairs_band([ref, ref], [qry, qry], 2, mode='extend', diagonals=[0, 5])
    with pytest.raises(hip.ClhError, match=r'pair 0: the band \[-9, -5\] of the 20 x 40 pair misses \(0, 0\)'):
        ssw_wrap.align_pairs_band([ref], [qry], 2, mode='prefix', diagonals=[-7])
    with pytest.raises(hip.ClhError, match=r'pair 1: the band \[-5, 5\] of the 40 x 20 pair has no end cell on row m \(lo > n - m = -20\)'):
        ssw_wrap.align_pairs_band([ref, qry], [qry, ref], 5, mode='prefix')
    assert ssw_wrap.align_pairs_band([qry], [ref], 5, mode='extend')[0].score == 40           # extend needs no cell of row m
    with pytest.raises(hip.ClhError, match=r'overlap with a band is not built'):
        _ctx().band_plan(hip.encode(qry), [0, 20], hip.encode(ref), [0, 40], hip.score_matrix(2, 2), 3, 1, 4, mode='overlap')
    with pytest.raises(hip.ClhError, match=r'pair 0: the clipped band \[-256, 256\] holds 513 diagonals.*full matrix'):
        ssw_wrap.align_pairs_band(['A' * 300], ['A' * 300], 256, mode='extend')


@pytest.mark.parametrize('mode', MODES)
def test_a_hinted_band(bgeom, mode):
    rng = chk.rng_for('gpu anchored hints', mode)
    rs = [chk.random_seq(rng, 200) for _ in range(6)]
    qs = [_flank(rng, r[d if d > 0 else 0:], 150, 120) if d >= 0 else chk.random_seq(rng, -d) + _flank(rng, r, 150, 120) for r, d in zip(rs, (0, 3, 8, -3, -8, 5))]
    wants = _check(_dna(qs), _dna(rs), chk.dna_matrix(10, 4), 8, 2, mode, band=8, diagonals=[0, 3, 8, -3, -8, 5])
    assert [x['band'] for x in wants] == [(-8, 8), (-5, 11), (0, 16), (-11, 5), (-16, 0), (-3, 13)]


@pytest.mark.parametrize('mode', MODES)
def test_certified_rows_equal_the_unbanded_kernel_on_the_same_device(bgeom, mode):
    rng = chk.rng_for('gpu anchored exact', mode)
    qs, rs = [], []
    for t in range(40):
        r = chk.random_seq(rng, rng.randint(30, 90))
        rs.append(r)
        if t % 3 == 0:                                           # one long gap: pushes the alignment to the band's edge or beyond
            at, g = rng.randint(5, 20), rng.randint(4, 14)
            qs.append(chk.mutate(rng, r[:at] + r[at + g:], 0.05) or 'A')
        else:
            qs.append(_flank(rng, r, rng.randint(20, len(r)), rng.randint(10, len(r))))
    mat = chk.dna_matrix(2, 2)
    w = 8
    keep = [k for k in range(40) if chk.refusal(mode, len(qs[k]), len(rs[k]), -w, w) is None]
    qs, rs = [qs[k] for k in keep], [rs[k] for k in keep]
    band = _rows(_dna(qs), _dna(rs), mat, 3, 1, mode, band=w)
    full = _rows(_dna(qs), _dna(rs), mat, 3, 1, mode)
    certified = [k for k in range(len(qs)) if band[k][7]]
    assert len(certified) >= 5 and len(certified) < len(qs) and any(band[k][:6] != full[k] for k in range(len(qs)))
    for k in certified:
        assert band[k][:6] == full[k], k


def test_a_3000_x_3000_extend_pair_in_one_mebibyte(bgeom):
    rng = chk.rng_for('gpu anchored 3000')
    ref = chk.random_seq(rng, 3000)
    qry = (chk.mutate(rng, ref[:2200], 0.08) + chk.random_seq(rng, 3000))[:3000]
    info = {}
    want, = _check(_dna([qry]), _dna([ref]), chk.dna_matrix(1, 3), 5, 2, 'extend', band=32, info=info, workspace_bytes=1 << 20)
    # under 1 / 3 / 5 / 2 unrelated letters lose: the extension ends where the copy does
    assert info['shares'] == 1 and info['max_pair_bytes'] <= 3000 * 66 // 2 + 16 and want['score'] > 1000 and 1900 < want['query_end'] < 2600


# ----------------------------------------------------------------------------------------------------------------------------
# extend_anchors
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def reads():
    return chk.anchored_reads(chk.rng_for('gpu anchors'), 200, seed_len=20)


@pytest.mark.parametrize('band', [None, 12])
def test_extend_anchors_on_reads_with_a_planted_seed(reads, band):
    from ciri_long_amd import ssw_wrap
    scoring = (2, 2, 3, 1)
    got = ssw_wrap.extend_anchors([x[0] for x in reads], [x[1] for x in reads], [x[2] for x in reads], band=band, seed_len=20,
                                  match=2, mismatch=2, gap_open=3, gap_extend=1, report_cigar=True)
    assert len(got) == 200
    exact = 0
    for (rs, qs, anchor), g in zip(reads, got):
        want, ex = chk.expected_anchor(rs, qs, anchor, 20, scoring, band)
        assert (g.score, g.ref_begin, g.ref_end, g.query_begin, g.query_end, g.cigar_string) == want[:5] + (chk.text_of(want, len(qs)),), anchor
        assert g.score >= 40 and g.ref_begin <= anchor[0] and g.ref_end >= anchor[0] + 19
        if band is not None:
            assert g.band_exact == bool(ex)
            exact += g.band_exact
    assert band is None or 20 < exact < 200
