"""The pair family against windows of the resident genome: K1g, K1gb, spliced alignment and extension from anchors with references
given as (contig, start, end, strand) and gathered on the device (csrc/genome.hip: genome_gather_kernel).  Everything is held to
the strings calls of the same process on the string the definition gives -- the window upper-cased, letters outside ACGT as N,
reversed and / or complemented -- row by row with CIGARs, and a sample of small pairs to the Python checkers."""
import re

import numpy as np
import pytest

import anchored_check as ac
import ends_check as ec
import spliced_check as sc
import twopiece_check as tc

pytestmark = pytest.mark.gpu

COMP = {'A': 'T', 'C': 'G', 'G': 'C', 'T': 'A', 'N': 'N'}
TWO = dict(match=2, mismatch=4, gap_open=4, gap_extend=2, gap_open2=24, gap_extend2=1)      # ssw_wrap.LONG_READ_GAPS
ONE = dict(match=2, mismatch=2, gap_open=3, gap_extend=1)

# the planted loci of the spliced test: three exons of 20 nt, introns of 497 and 700 letters, in a window of 1300
EXON_AT = (20, 20 + 20 + 497, 20 + 20 + 497 + 20 + 700)


def _locus(rng, minus):
    """(window string of 1300 letters, the query) -- GT..AG introns on '+', CT..AC on '-'; intron bodies are soft-masked"""
    exons = [ec.random_seq(rng, 20) for _ in range(3)]
    body = lambda n: ec.random_seq(rng, n - 4, 'AGT' if minus else 'ACT').lower()
    i1 = ('CT' + body(497) + 'AC') if minus else ('GT' + body(497) + 'AG')
    i2 = ('CT' + body(700) + 'AC') if minus else ('GT' + body(700) + 'AG')
    core = exons[0] + i1 + exons[1] + i2 + exons[2]
    w = ec.random_seq(rng, 20, 'AT') + core + ec.random_seq(rng, 1300 - 20 - len(core), 'AT')
    assert len(w) == 1300
    return w, ''.join(exons)


@pytest.fixture(scope='module')
def world():
    """one genome of three contigs, about 40 kb: lower-case stretches, N runs, letters outside the alphabet, a contig of one base"""
    from ciri_long_amd import hip
    rng = ec.rng_for('gpu windows pairs')
    a = ec.random_seq(rng, 25000)
    a = a[:3000] + a[3000:4200].lower() + a[4200:9000] + 'N' * 300 + a[9300:12000] + ec.random_seq(rng, 500, 'ACGTacgtNnRY-') + a[12500:]
    plus, q_plus = _locus(rng, False)
    minus, q_minus = _locus(rng, True)
    a = a[:15003] + plus + a[16303:19001] + minus + a[20301:]
    b = ec.random_seq(rng, 14000)
    b = b[:17].lower() + b[17:5000] + b[5000:5700].lower() + b[5700:8000] + 'n' * 40 + b[8040:13990] + b[13990:].lower()
    contigs = {'chrA': a, 'one': 'g', 'chrB': b}
    assert len(a) == 25000 and len(b) == 14000
    ctx = hip.default_context()
    g = hip.Genome(ctx, contigs)
    yield dict(contigs=contigs, genome=g, ctx=ctx, loci=dict(plus=(15003, q_plus), minus=(19001, q_minus)))
    g.close()


def _string(contigs, ctg, a, b, flags):
    """the definition: upper-cased, letters outside ACGT as N, then reversed (bit 0) and / or complemented (bit 1)"""
    s = ''.join(c if c in 'ACGT' else 'N' for c in contigs[ctg][a:b].upper())
    if flags & 1:
        s = s[::-1]
    if flags & 2:
        s = ''.join(COMP[c] for c in s)
    return s


def _tup(r):
    return (r.score, r.ref_begin, r.ref_end, r.query_begin, r.query_end, r.cigar_string)


def _rows(rows, cig):
    return [tuple(int(r[f]) for f in ('score', 'ref_begin', 'ref_end', 'query_begin', 'query_end')) +
            (tuple(int(c) for c in cig[int(r['cigar_off']):int(r['cigar_off']) + int(r['cigar_len'])]),) for r in rows]


def _coords_ok(res, ctg, a, b, minus):
    L = b - a
    want = (a + L - 1 - res.ref_end, a + L - 1 - res.ref_begin) if minus else (a + res.ref_begin, a + res.ref_end)
    assert (res.contig, res.minus, res.genome_begin, res.genome_end) == (ctg, bool(minus), want[0], want[1])


def _tile():
    import os
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return int(re.search(r'kGatherTile = (\d+);', open(os.path.join(here, 'ciri_long_amd', 'csrc', 'genome_gather.h')).read()).group(1))


# ---- 1. the gather alone, through the plans -------------------------------------------------------------------------------------
def test_gather_every_offset_length_and_flag_through_a_global_plan(world):
    from ciri_long_amd import hip, ssw_wrap
    contigs, g, ctx = world['contigs'], world['genome'], world['ctx']
    tile = _tile()
    wins = []
    for off in range(16):
        for L in (0, 1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 511, 512, 513):
            wins.append(('chrA', 2990 + off, 2990 + off + L))      # across the upper / lower case edge at 3000
    for L in (tile - 1, tile, tile + 1):
        for off in (0, 5, 11):
            wins.append(('chrB', 4000 + off, 4000 + off + L))
    for ctg in ('chrA', 'chrB'):                                                     # contig starts and ends: the genome's first and last bytes among them
        n = len(contigs[ctg])
        wins += [(ctg, 0, L) for L in (1, 15, 16, 17, 65)] + [(ctg, n - L, n) for L in (1, 15, 16, 17, 65)]
    wins += [('one', 0, 1), ('one', 0, 0), ('one', 1, 1), ('chrA', 8990, 9320), ('chrA', 11990, 12510), ('chrB', 7990, 8050)]      # N runs, odd letters
    off, ln = ssw_wrap._window_spans('test', g, wins)
    mat = hip.score_matrix(2, 2)
    for flags in range(4):
        strings = [_string(contigs, c, a, b, flags) for c, a, b in wins]
        qd, qo = hip.pack(strings)
        got = _rows(*ctx.ends_batch(qd, qo, None, None, mat, 3, 1, mode='global', want_cigar=True,
                                    windows=(g, off, ln, np.full(len(wins), flags, dtype=np.uint8))))
        rd, ro = hip.pack(strings)
        want = _rows(*ctx.ends_batch(qd, qo, rd, ro, mat, 3, 1, mode='global', want_cigar=True))
        assert got == want, flags
        for s, row in zip(strings, got):
            if 'N' not in s:
                assert row[0] == 2 * len(s) and row[5] == (((len(s) << 4),) if s else ()), (flags, len(s))
        if flags in (0, 3):      # the public call: minus is flags 3
            res = ssw_wrap.align_windows_ends(g, wins, [flags == 3] * len(wins), strings, mode='global', report_cigar=True)
            ref = ssw_wrap.align_pairs_ends(strings, strings, mode='global', report_cigar=True)
            assert [_tup(r) for r in res] == [_tup(r) for r in ref]
            for r, (c, a, b) in zip(res, wins):
                _coords_ok(r, c, a, b, flags == 3)


# ---- 2. K1g ---------------------------------------------------------------------------------------------------------------------
def _random_pairs(world, rng, count, wlo, whi, qlo, qhi, small=0):
    """windows of wlo..whi letters on both strands with a query of qlo..qhi letters mutated from inside each; the first `small`
    windows are at most 150 letters, for the Python checkers"""
    contigs = world['contigs']
    wins, minus, queries, strings = [], [], [], []
    for k in range(count):
        ctg = 'chrA' if k % 3 else 'chrB'
        L = rng.randint(wlo, min(whi, 150) if k < small else whi)
        a = rng.randrange(0, len(contigs[ctg]) - L)
        mn = bool(k & 1)
        s = _string(contigs, ctg, a, a + L, 3 if mn else 0)
        ql = min(rng.randint(qlo, qhi), L)
        p = rng.randrange(0, L - ql + 1)
        q = ec.mutate(rng, s[p:p + ql].replace('N', 'A'), 0.12) or 'A'
        wins.append((ctg, a, a + L)); minus.append(mn); queries.append(q); strings.append(s)
    return wins, minus, queries, strings


def _checker(mode, q, r, kw):
    mat = ec.dna_matrix(kw['match'], kw['mismatch'])
    qc, rc = ec.encode(q), ec.encode(r)
    if 'gap_open2' in kw:
        return tc.align(qc, rc, mat, (kw['gap_open'], kw['gap_extend'], kw['gap_open2'], kw['gap_extend2']), mode)
    return (ac if mode in ac.MODES else ec).align(qc, rc, mat, kw['gap_open'], kw['gap_extend'], mode)


def _text(want, m):
    head = '%dS' % want['query_begin'] if want['query_begin'] > 0 else ''
    tail = m - want['query_end'] - 1
    return head + ec.cigar_text(want['cigar']) + ('%dS' % tail if tail else '')


@pytest.mark.parametrize('kw', [ONE, TWO], ids=['one-piece', 'two-piece'])
def test_ends_five_modes_equal_the_strings_call_and_the_checkers(world, kw):
    from ciri_long_amd import ssw_wrap
    g = world['genome']
    chunks = set()
    for mode in ('global', 'semiglobal', 'overlap', 'prefix', 'extend'):
        wins, minus, queries, strings = _random_pairs(world, ec.rng_for('gpu windows ends', mode, len(kw)), 24, 60, 1100, 40, 130, small=4)
        got = ssw_wrap.align_windows_ends(g, wins, minus, queries, mode=mode, report_cigar=True, traceback='stored', **kw)
        want = ssw_wrap.align_pairs_ends(strings, queries, mode=mode, report_cigar=True, traceback='stored', **kw)
        assert [_tup(r) for r in got] == [_tup(r) for r in want], mode
        for r, (c, a, b), mn in zip(got, wins, minus):
            _coords_ok(r, c, a, b, mn)
            chunks.add((b - a + 511) // 512)
        for k in range(4):                                   # 5 modes x 2 cost sets x 4 = 40 small pairs against the definitions
            chk = _checker(mode, queries[k], strings[k], kw)
            assert _tup(got[k]) == ec.as_tuple(chk)[:5] + (_text(chk, len(queries[k])),), (mode, k)
    assert chunks >= {1, 2, 3}


def test_ends_stored_and_recompute_routes_and_a_plan_cut_into_shares(world):
    from ciri_long_amd import hip, ssw_wrap
    g, ctx = world['genome'], world['ctx']
    wins, minus, queries, strings = _random_pairs(world, ec.rng_for('gpu windows routes'), 24, 200, 1300, 60, 130)
    assert {(b - a + 511) // 512 for _, a, b in wins} == {1, 2, 3}
    want = [_tup(r) for r in ssw_wrap.align_pairs_ends(strings, queries, mode='global', report_cigar=True, **ONE)]
    for route in ('stored', 'recompute'):
        got = ssw_wrap.align_windows_ends(g, wins, minus, queries, mode='global', report_cigar=True, traceback=route, **ONE)
        assert [_tup(r) for r in got] == want, route
    # one plan whose workspace holds the largest pair alone: several shares, the same rows
    off, ln = ssw_wrap._window_spans('test', g, wins)
    flags = np.where(np.array(minus), 3, 0).astype(np.uint8)
    qd, qo = hip.pack(queries)
    mat = hip.score_matrix(2, 2)
    whole = hip.EndsPlan(ctx, qd, qo, None, None, mat, 3, 1, mode='global', windows=(g, off, ln, flags))
    whole.run(); rows = _rows(*whole.fetch()); info = whole.info(); whole.close()
    cut = hip.EndsPlan(ctx, qd, qo, None, None, mat, 3, 1, mode='global', workspace_bytes=info['max_pair_bytes'], windows=(g, off, ln, flags))
    cut.run(); cut_rows = _rows(*cut.fetch()); cut_info = cut.info()
    cut.run(); again = _rows(*cut.fetch()); cut.close()                            # the gather ran at create: a second run reads the same buffer
    assert info['shares'] == 1 and cut_info['shares'] > 1 and cut_info['workspace_bytes'] <= info['max_pair_bytes']
    assert rows == cut_rows == again
    assert [r[:5] for r in rows] == [t[:5] for t in want]


# ---- 3. K1gb --------------------------------------------------------------------------------------------------------------------
def _band_cases(world, mode):
    """(window, minus, query, band, diagonal or None): clipped widths 1, 127, 128, 129 and 512 without a hint, and hinted bands"""
    rng, contigs = ec.rng_for('gpu windows band', mode), world['contigs']
    anchored = mode in ('prefix', 'extend')
    shapes = [(50, 50, 0), (300, 301, 255)] if not anchored else [(50, 60, 0), (255, 300, 256)]
    shapes += [(200, 200 + d, 63) for d in (0, 1, 2)] if not anchored else [(63, 90, 64), (64, 90, 64), (200, 210, 63)]
    out = []
    for k, (m, n, band) in enumerate(shapes * 2):
        ctg = 'chrB' if k % 2 else 'chrA'
        a = rng.randrange(0, len(contigs[ctg]) - n)
        mn = k >= len(shapes)
        s = _string(contigs, ctg, a, a + n, 3 if mn else 0)
        q = (ec.mutate(rng, s.replace('N', 'A'), 0.06) + ec.random_seq(rng, m))[:m]
        out.append(((ctg, a, a + n), mn, q, band, None))
    if mode == 'semiglobal':      # a placement known: the diagonal is reference position minus query position
        for k in range(8):
            n, m = rng.randint(400, 900), rng.randint(60, 120)
            a = rng.randrange(0, len(contigs['chrA']) - n)
            mn = bool(k & 1)
            s = _string(contigs, 'chrA', a, a + n, 3 if mn else 0)
            p = rng.randrange(0, n - m)
            out.append((('chrA', a, a + n), mn, ec.mutate(rng, s[p:p + m].replace('N', 'A'), 0.1) or 'A', 20, p))
    return out


@pytest.mark.parametrize('mode', ['global', 'semiglobal', 'prefix', 'extend'])
def test_band_equals_the_strings_call(world, mode):
    from ciri_long_amd import ssw_wrap
    g, contigs = world['genome'], world['contigs']
    cases = _band_cases(world, mode)
    widths = set()
    for band in sorted({c[3] for c in cases}):
        for hinted in (False, True):
            sel = [c for c in cases if c[3] == band and (c[4] is not None) == hinted]
            if not sel:
                continue
            wins, minus, queries = [c[0] for c in sel], [c[1] for c in sel], [c[2] for c in sel]
            diags = [c[4] for c in sel] if hinted else None
            strings = [_string(contigs, c, a, b, 3 if mn else 0) for (c, a, b), mn in zip(wins, minus)]
            for kw in (ONE, TWO):
                got = ssw_wrap.align_windows_band(g, wins, minus, queries, band, mode=mode, diagonals=diags, report_cigar=True, **kw)
                want = ssw_wrap.align_pairs_band(strings, queries, band, mode=mode, diagonals=diags, report_cigar=True, **kw)
                assert [_tup(r) + (r.band, r.band_exact) for r in got] == [_tup(r) + (r.band, r.band_exact) for r in want], (mode, band, hinted)
            for r, (c, a, b), mn in zip(got, wins, minus):
                _coords_ok(r, c, a, b, mn)
                widths.add(r.band[1] - r.band[0] + 1)
    assert widths >= {1, 127, 128, 129, 512}, widths


# ---- 4. spliced -----------------------------------------------------------------------------------------------------------------
def test_spliced_planted_exons_on_both_strands(world):
    from ciri_long_amd import ssw_wrap
    g, contigs = world['genome'], world['contigs']
    (ap, qp), (am, qm) = world['loci']['plus'], world['loci']['minus']
    wins = [('chrA', ap, ap + 1300), ('chrA', am, am + 1300)]
    queries, strands = [qp, qm], ['+', '-']
    strings = [_string(contigs, c, a, b, 0) for c, a, b in wins]
    planted = lambda a: [(a + e, a + e + 19) for e in EXON_AT]
    for route in ('stored', 'recompute'):
        got = ssw_wrap.align_windows_spliced(g, wins, queries, strand=strands, report_cigar=True, traceback=route)
        want = ssw_wrap.align_pairs_spliced(strings, queries, strand=strands, report_cigar=True, traceback=route)
        assert [_tup(r) + (r.strand,) for r in got] == [_tup(r) + (r.strand,) for r in want]
        for r, (c, a, b), s in zip(got, wins, strands):
            assert r.cigar_string == '20M497N20M700N20M' and r.score == 2 * 60 - 2 * 12 and r.strand == s
            assert r.exons == planted(a) and (r.genome_begin, r.genome_end) == (a + 20, a + 1276) and not r.minus
    both = ssw_wrap.align_windows_spliced(g, wins, queries, strand='both', report_cigar=True)
    ref = ssw_wrap.align_pairs_spliced(strings, queries, strand='both', report_cigar=True)
    assert [_tup(r) + (r.strand,) for r in both] == [_tup(r) + (r.strand,) for r in ref]
    assert [r.strand for r in both] == ['+', '-'] and [r.exons for r in both] == [planted(ap), planted(am)]
    costs, mat = sc.make_costs(), sc.dna_matrix(2, 2)
    for r, s, q, st in zip(both, strings, queries, (1, -1)):
        chk = sc.align(sc.encode(q), sc.encode(s), mat, costs, 'semiglobal', st)
        assert _tup(r) == sc.as_tuple(chk)[:5] + (_text(chk, len(q)),)


def test_spliced_empty_query_in_global_mode_is_the_row0_intron_row(world):
    """no query letter: the window costs one deletion or, where that is dearer, one intron whose sites are the window's first two and
    last two letters -- which the create reads back from what the gather wrote"""
    from ciri_long_amd import ssw_wrap
    g, contigs = world['genome'], world['contigs']
    ap, am = world['loci']['plus'][0], world['loci']['minus'][0]
    wins = [('chrA', ap + 40, ap + 40 + 497), ('chrA', am + 40, am + 40 + 497),      # the planted introns themselves: GT..AG and CT..AC
            ('chrA', ap + 41, ap + 40 + 497), ('chrA', 100, 130), ('chrA', 100, 102), ('chrA', 100, 101), ('one', 0, 1), ('chrA', 9100, 9120)]
    queries = [''] * len(wins)
    strings = [_string(contigs, c, a, b, 0) for c, a, b in wins]
    costs, mat = sc.make_costs(), sc.dna_matrix(2, 2)
    for strand, st in (('+', 1), ('-', -1)):
        got = ssw_wrap.align_windows_spliced(g, wins, queries, mode='global', strand=strand, report_cigar=True)
        want = ssw_wrap.align_pairs_spliced(strings, queries, mode='global', strand=strand, report_cigar=True)
        assert [_tup(r) for r in got] == [_tup(r) for r in want]
        for r, s in zip(got, strings):
            chk = sc.align(sc.encode(''), sc.encode(s), mat, costs, 'global', st)
            assert _tup(r) == sc.as_tuple(chk)[:5] + (_text(chk, 0),)
        canonical = got[0] if st > 0 else got[1]
        assert (canonical.score, canonical.cigar_string) == (-12, '497N')
        assert canonical.exons == []


# ---- 5. extension from anchors ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('band', [None, 24])
def test_extend_anchors_genome_equals_extend_anchors_on_the_flank_strings(world, band):
    from ciri_long_amd import ssw_wrap
    g, contigs, rng = world['genome'], world['contigs'], ec.rng_for('gpu windows anchors', band)
    anchors, minus, queries, refs, local = [], [], [], [], []
    spots = [('chrB', p) for p in (0, 3, 40, 7000, 13960, 13997, 14000)] + [('chrA', p) for p in (0, 25, 3010, 9150, 24990, 25000)] + [('one', 0), ('one', 1)]
    slack = 64 if band is None else band
    for k, (ctg, pos) in enumerate(spots * 2):
        mn = k >= len(spots)
        n = len(contigs[ctg])
        # a query read off the strand around pos, mutated; its anchor letter sits where pos does
        lo, hi = max(0, pos - rng.randint(0, 90)), min(n, pos + rng.randint(0, 90))
        s = _string(contigs, ctg, lo, hi, 3 if mn else 0)
        cut = (hi - pos) if mn else (pos - lo)
        left_q, right_q = ec.mutate(rng, s[:cut].replace('N', 'A'), 0.08), ec.mutate(rng, s[cut:].replace('N', 'A'), 0.08)
        q, qp = left_q + right_q, len(left_q)
        left, right, start = ssw_wrap._anchor_flanks(n, pos, qp, len(q), slack, mn)
        anchors.append((ctg, pos, qp)); minus.append(mn); queries.append(q)
        refs.append(_string(contigs, ctg, start, start + left + right, 3 if mn else 0)); local.append((left, qp))
    for kw in (ONE, TWO):
        got = ssw_wrap.extend_anchors_genome(g, anchors, minus, queries, band=band, report_cigar=True, **kw)
        want = ssw_wrap.extend_anchors(refs, queries, local, band=band, report_cigar=True, **kw)
        for k, (a, b) in enumerate(zip(got, want)):
            assert _tup(a) == _tup(b), (k, anchors[k], minus[k])
            if band is not None:
                assert a.band_exact == b.band_exact
            ctg, pos, _ = anchors[k]
            left, right, start = ssw_wrap._anchor_flanks(len(contigs[ctg]), pos, anchors[k][2], len(queries[k]), slack, minus[k])
            _coords_ok(a, ctg, start, start + left + right, minus[k])
    assert any(r.score > 40 for r in got)


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals(world):
    from ciri_long_amd import hip, ssw_wrap
    g, ctx, contigs = world['genome'], world['ctx'], world['contigs']
    total = sum(len(s) for s in contigs.values())
    qd, qo = hip.pack(['ACGT', 'ACGT'])
    mat = hip.score_matrix(2, 2)
    plan = lambda off, ln, flags, cls=hip.EndsPlan, m=mat, **kw: (
        cls(ctx, qd, qo, None, None, m, 3, 1, windows=(g, off, ln, flags), **kw) if cls is hip.EndsPlan else
        cls(ctx, qd, qo, None, None, m, 3, 1, 8, windows=(g, off, ln, flags), **kw))
    for cls in (hip.EndsPlan, hip.BandPlan):
        with pytest.raises(hip.ClhError, match=r'pair 1: the window \[%d, %d \+ 8\) lies outside the genome of %d bases' % (total - 7, total - 7, total)):
            plan([0, total - 7], [8, 8], [0, 0], cls)
        with pytest.raises(hip.ClhError, match=r'pair 1: the window'):
            plan([0, 10], [8, -1], [0, 0], cls)
        with pytest.raises(hip.ClhError, match=r'pair 0: the window'):
            plan([-1, 10], [8, 8], [0, 0], cls)
        with pytest.raises(hip.ClhError, match=r'pair 1: window flags must be 0\.\.3 .* got 4'):
            plan([0, 10], [8, 8], [3, 4], cls)
        # a 24-letter matrix: CLH_E_UNSUPPORTED, matrices on genome windows stay DNA only
        with pytest.raises(hip.ClhError, match=r'windows of the resident genome are DNA codes: the matrix must be 5 x 5, n_mat is 24'):
            plan([0, 10], [8, 8], [0, 0], cls, m=np.ones(24 * 24, dtype=np.int8))
        with pytest.raises(ValueError, match='either refs and ref_off or windows, not both'):
            if cls is hip.EndsPlan:
                cls(ctx, qd, qo, qd, qo, mat, 3, 1, windows=(g, [0, 10], [8, 8], [0, 0]))
            else:
                cls(ctx, qd, qo, qd, qo, mat, 3, 1, 8, windows=(g, [0, 10], [8, 8], [0, 0]))
        ok = plan([0, total - 8], [8, 8], [0, 3], cls)       # the last window ends at the genome's last byte
        ok.run(); ok.fetch(); ok.close()
    L = hip.lib()
    opts = hip.EndsOpts(hip.ENDS_MODES['global'], mat.ctypes.data, 5, 3, 1, 1, 0)
    assert not L.clh_ends_plan_create_windows(None, 0, None, qo.ctypes.data, None, None, None, opts, None, None, None)
    assert 'null genome' in hip.last_error()
    with pytest.raises(ValueError, match=r"window 0 \('chrA', 24990, 25001\)"):
        ssw_wrap.align_windows_ends(g, [('chrA', 24990, 25001)], [False], ['ACGT'])


# ---- 7. the lower-case rule -------------------------------------------------------------------------------------------------------
def test_a_soft_masked_minus_strand_window_aligns_here_and_not_on_the_local_path(world):
    """lower-case bases are complemented by the gather; Genome.ssw_windows keeps the reference's revcomp() quirk and leaves them"""
    from ciri_long_amd import ssw_wrap
    g, contigs = world['genome'], world['contigs']
    win = ('chrA', 3100, 3400)                       # inside the lower-case stretch
    raw = contigs['chrA'][3100:3400]
    assert raw == raw.lower() and set(raw) <= set('acgt')
    q = ''.join(COMP[c] for c in reversed(raw.upper()))      # its true reverse complement
    here = ssw_wrap.align_windows_ends(g, [win], [True], [q], mode='global', report_cigar=True)[0]
    assert (here.score, here.cigar_string) == (2 * 300, '300M')
    there = ssw_wrap.align_windows(g, [win], [True], [q], report_cigar=True)[0]
    assert there is None or there.score < 2 * 300 // 2
