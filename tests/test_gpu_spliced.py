"""Spliced pair alignment on the GPU: K1g with intron gaps (csrc/ssw_ends.hip), all five modes.  Every expected value is
tests/spliced_check.py (`align`), field by field with CIGARs, through the storing route and the score-only route, and every CIGAR is
rescored on its own; with an intron too dear to win the rows are also held to align_pairs_ends of the same device."""
import ctypes as C

import numpy as np
import pytest

import spliced_check as chk

pytestmark = pytest.mark.gpu

MODES = chk.MODES
DEFAULT = dict(go=3, ge=1, io=12, noncanonical=6)
CHEAP = dict(go=3, ge=1, io=1, noncanonical=1)          # a one-letter run is already cheaper as an intron where a site is canonical
TIE = dict(go=3, ge=1, io=4, noncanonical=0)            # two letters: deletion 4, intron 4


def _ctx():
    from ciri_long_amd import hip
    return hip.default_context()


def _text(want, m):
    head = '%dS' % want['query_begin'] if want['query_begin'] > 0 else ''
    tail = m - want['query_end'] - 1
    return head + chk.cigar_text(want['cigar']) + ('%dS' % tail if tail else '')


def _hip_rows(rows, cig):
    return [(int(r['score']), int(r['ref_begin']), int(r['ref_end']), int(r['query_begin']), int(r['query_end']),
             chk.cigar_text([('MIDN'[int(c) & 15], int(c) >> 4) for c in cig[int(r['cigar_off']):int(r['cigar_off']) + int(r['cigar_len'])]]))
            for r in rows]


def _kw(kw):
    return dict(gap_open=kw['go'], gap_extend=kw['ge'], intron_open=kw['io'], noncanonical=kw['noncanonical'],
                donor_costs=kw.get('donor'), acceptor_costs=kw.get('acceptor'))


def _check(refs, queries, mode, kw=DEFAULT, strands=None, wants=None):
    """align_pairs_spliced against the checker, field by field, storing route and score-only route; every CIGAR is also rescored on
    its own -> the checker's results"""
    from ciri_long_amd import hip, ssw_wrap
    costs = chk.make_costs(**kw)
    mat = chk.dna_matrix(2, 2)
    strands = list(strands) if strands is not None else [1] * len(refs)
    got = ssw_wrap.align_pairs_spliced(refs, queries, mode=mode, strand=['+' if s > 0 else '-' for s in strands], report_cigar=True, **_kw(kw))
    assert len(got) == len(refs)
    if wants is None:
        wants = [chk.align(chk.encode(qs), chk.encode(rs), mat, costs, mode, s) for rs, qs, s in zip(refs, queries, strands)]
    for k, (rs, qs, s, g, want) in enumerate(zip(refs, queries, strands, got, wants)):
        have = (g.score, g.ref_begin, g.ref_end, g.query_begin, g.query_end, g.cigar_string)
        assert have == chk.as_tuple(want)[:5] + (_text(want, len(qs)),), (k, mode, kw, s, len(qs), len(rs))
        assert g.strand == ('+' if s > 0 else '-')
        ops = [(o, n) for o, n in chk.parse_cigar(g.cigar_string) if o != 'S']
        chk.check_cigar(dict(score=g.score, ref_begin=g.ref_begin, ref_end=g.ref_end, query_begin=g.query_begin, query_end=g.query_end, cigar=ops),
                        chk.encode(qs), chk.encode(rs), mat, costs, mode, s)
    # the score-only route: another instantiation of the kernel, no stored decisions, no walk
    qd, qo = hip.pack(queries); rd, ro = hip.pack(refs)
    sp = hip.splice_of('test', kw['io'], kw['noncanonical'], kw.get('donor'), kw.get('acceptor'))
    rows, cig = _ctx().ends_batch(qd, qo, rd, ro, hip.score_matrix(2, 2), kw['go'], kw['ge'], mode=mode, want_cigar=False, splice=sp,
                                  strand=np.array(strands, dtype=np.int8))
    assert len(cig) == 0
    for k, want in enumerate(wants):
        assert (int(rows[k]['score']), int(rows[k]['ref_end']), int(rows[k]['query_end'])) == (want['score'], want['ref_end'], want['query_end']), (k, mode, kw)
    return wants


def revcomp(s):
    return ''.join({'A': 'T', 'C': 'G', 'G': 'C', 'T': 'A', 'N': 'N'}[c] for c in reversed(s))


def _intron(rng, length):
    """GT + letters over ACT + AG; below 4 letters what fits of GT..AG"""
    if length < 4:
        return 'GTAG'[:length] if length != 2 else 'GT'
    return 'GT' + chk.random_seq(rng, length - 4, 'ACT') + 'AG'


def _edge_cases(rng):
    """(mode, query, reference, wants an N): introns whose first letter, and whose last letter, sits at the 1-based columns 1, 7, 8, 9,
    511, 512, 513 and n"""
    out = []
    ex = lambda k: chk.random_seq(rng, k)
    for first in (1, 7, 8, 9, 511, 512, 513):
        e1, e2 = ex(min(20, first - 1)), ex(20)
        fill = chk.random_seq(rng, first - 1 - len(e1), 'AT')
        out.append(('semiglobal' if fill else 'global', e1 + e2, fill + e1 + _intron(rng, 40) + e2, True))
    for last in (1, 7, 8, 9):                              # a leading run: row 0 of the anchored modes
        e2 = ex(20)
        out.append(('global', e2, _intron(rng, last) + e2, False))
        out.append(('prefix', e2, _intron(rng, last) + e2 + 'CA', False))
    for last in (511, 512, 513):
        e1, e2 = ex(20), ex(20)
        fill = chk.random_seq(rng, last - 60, 'AT')
        out.append(('semiglobal', e1 + e2, fill + e1 + _intron(rng, 40) + e2 + 'TC', True))
    e1 = ex(20)
    out.append(('global', e1, e1 + 'G', False))            # the first letter at column n: the start dinucleotide runs off the reference
    out.append(('global', e1, e1 + _intron(rng, 40), True))        # a trailing intron: its last letter at column n
    out.append(('global', e1, e1[:12] + _intron(rng, 30) + e1[12:] + _intron(rng, 25), True))
    return out


@pytest.mark.parametrize('kw', [DEFAULT, CHEAP], ids=['default', 'cheap'])
def test_introns_that_begin_and_end_at_lane_edges_chunk_edges_column_1_and_column_n(kw):
    rng = chk.rng_for('gpu spliced edges')
    cases = _edge_cases(rng)
    for mode in ('global', 'semiglobal', 'prefix'):
        sel = [c for c in cases if c[0] == mode]
        wants = _check([c[2] for c in sel], [c[1] for c in sel], mode, kw)
        for c, w in zip(sel, wants):
            if c[3] and kw is DEFAULT:
                assert 'N' in chk.cigar_text(w['cigar']), (c[0], len(c[2]), w['cigar'])
        # the same pairs from the other strand: every position mirrored
        _check([revcomp(c[2]) for c in sel], [revcomp(c[1]) for c in sel], mode, kw, strands=[-1] * len(sel))
    if kw is CHEAP:      # the one-letter runs at column 1 and at column n are introns here, with `other` for the dinucleotide off the reference
        costs = chk.make_costs(**kw)
        w = _check(['ACGTAAG', 'ACGTACG'], ['ACGTAA', 'ACGTAC'], 'global', kw)
        assert (chk.cigar_text(w[0]['cigar']), w[0]['score']) == ('6M1N', 12 - (1 + 1 + 0))      # start: off the reference; end: AG
        assert (chk.cigar_text(w[1]['cigar']), w[1]['score']) == ('6M1D', 12 - 3)                # 1 + 1 + 1 ties with the deletion


def literal_case():
    exons = ('ACGTTACGGATCCATGCAAT', 'TTCGAGGCTAACCGTATGCA', 'GGATTCACCGTAGCTAGCAT')
    rng = chk.rng_for('spliced literal')
    i1 = 'GT' + chk.random_seq(rng, 493, 'ACT') + 'AG'
    i2 = 'GT' + chk.random_seq(rng, 696, 'ACT') + 'AG'
    return ''.join(exons), 'CCTA' + exons[0] + i1 + exons[1] + i2 + exons[2] + 'TTAC'


def test_three_exons_two_introns_both_strands_and_both():
    from ciri_long_amd import align, ssw_wrap
    qs, rs = literal_case()
    wants = _check([rs, revcomp(rs), revcomp(rs)], [qs, revcomp(qs), revcomp(qs)], 'semiglobal', strands=[1, -1, 1])
    assert chk.as_tuple(wants[0]) == (96, 4, len(rs) - 5, 0, 59, '20M497N20M700N20M')
    assert chk.as_tuple(wants[1]) == (96, 4, len(rs) - 5, 0, 59, '20M700N20M497N20M')
    assert wants[2]['score'] < 96
    both = ssw_wrap.align_pairs_spliced([rs, revcomp(rs), 'ACGTACGT'], [qs, revcomp(qs), 'ACGTACGT'], strand='both', report_cigar=True)
    assert [(b.score, b.strand, b.cigar_string) for b in both] == [(96, '+', '20M497N20M700N20M'), (96, '-', '20M700N20M497N20M'), (16, '+', '8M')]
    # what align.py makes of it
    import types
    hit = types.SimpleNamespace(r_st=both[0].ref_begin, q_st=0, cigar=align.convert_cigar_string(both[0].cigar_string))
    assert align.get_exons(hit) == [[4, 24, 0, 20], [521, 541, 20, 40], [1241, 1261, 40, 60]]
    assert [b[:2] for b in align.get_blocks(hit)] == [[4, 24], [521, 541], [1241, 1261]]


def test_both_is_the_better_of_the_two_strands_ties_to_plus():
    from ciri_long_amd import ssw_wrap
    rng = chk.rng_for('gpu spliced both')
    refs, queries = [], []
    for k in range(24):
        e1, e2 = chk.random_seq(rng, 15), chk.random_seq(rng, 15)
        rs = chk.random_seq(rng, 9) + e1 + _intron(rng, rng.randint(20, 90)) + e2 + chk.random_seq(rng, 5)
        qs = chk.mutate(rng, e1 + e2, 0.06) or 'A'
        if k % 3 == 1:
            rs, qs = revcomp(rs), revcomp(qs)
        if k % 3 == 2:
            rs = rs.replace('GT', 'GA').replace('AG', 'AC')
        refs.append(rs); queries.append(qs)
    for mode in ('semiglobal', 'global'):
        plus = ssw_wrap.align_pairs_spliced(refs, queries, mode=mode, strand='+', report_cigar=True)
        minus = ssw_wrap.align_pairs_spliced(refs, queries, mode=mode, strand='-', report_cigar=True)
        both = ssw_wrap.align_pairs_spliced(refs, queries, mode=mode, strand='both', report_cigar=True)
        picked = set()
        for p, m_, b in zip(plus, minus, both):
            w = p if p.score >= m_.score else m_
            assert (b.score, b.strand, b.ref_begin, b.ref_end, b.cigar_string) == (w.score, w.strand, w.ref_begin, w.ref_end, w.cigar_string)
            picked.add(b.strand)
        assert picked == {'+', '-'}
    _check(refs, queries, 'semiglobal', strands=[1 if k % 2 else -1 for k in range(len(refs))])      # a per-pair mix in one plan


def test_an_intron_that_spans_two_whole_chunks():
    rng = chk.rng_for('gpu spliced span')
    e1, e2 = chk.random_seq(rng, 40), chk.random_seq(rng, 40)
    rs = chk.random_seq(rng, 20) + e1 + _intron(rng, 1450) + e2 + chk.random_seq(rng, 50)
    assert 1590 <= len(rs) <= 1610
    qs = chk.mutate(rng, e1 + e2, 0.05)
    for mode in MODES:
        wants = _check([rs, revcomp(rs)], [qs, revcomp(qs)], mode, strands=[1, -1])
        if mode in ('semiglobal', 'overlap'):
            assert '1450N' in chk.cigar_text(wants[0]['cigar']) and '1450N' in chk.cigar_text(wants[1]['cigar'])


@pytest.mark.parametrize('mode', ['global', 'prefix', 'extend'])
def test_an_intron_on_row_0_of_an_anchored_mode_and_a_trailing_one(mode):
    rng = chk.rng_for('gpu spliced row0', mode)
    refs, queries = [], []
    for lead in (5, 13, 14, 60, 530, 1030):
        e = chk.random_seq(rng, 30)
        refs.append(_intron(rng, lead) + e + ('' if mode == 'global' else 'TTC')); queries.append(e)
        refs.append(e + _intron(rng, lead)); queries.append(e)
    wants = _check(refs, queries, mode)
    _check(refs, queries, mode, CHEAP)
    _check([revcomp(r) for r in refs], [revcomp(q) for q in queries], mode, strands=[-1] * len(refs))
    if mode != 'extend':
        assert chk.cigar_text(wants[0]['cigar']) == '5D30M' and chk.cigar_text(wants[6]['cigar']) == '60N30M'       # 3 + 4 < 12 and 3 + 59 > 12
    if mode == 'global':
        assert chk.cigar_text(wants[7]['cigar']) == '30M60N'


def test_ties_between_a_deletion_and_an_intron_resolve_to_d():
    rng = chk.rng_for('gpu spliced tie')
    refs, queries = [], []
    for _ in range(60):
        qs = chk.random_seq(rng, rng.randint(2, 12), 'AG')
        at = rng.randint(0, len(qs))
        refs.append(qs[:at] + chk.random_seq(rng, rng.randint(1, 3), 'T') + qs[at:]); queries.append(qs)
    for mode in MODES:
        wants = _check(refs, queries, mode, TIE)
    wants = _check(refs, queries, 'global', TIE)
    assert any(('D', 2) in w['cigar'] for w in wants) and any(('N', 3) in w['cigar'] for w in wants)
    assert not any(('N', 2) in w['cigar'] or ('N', 1) in w['cigar'] for w in wants)


def test_cigars_with_as_many_runs_as_the_host_reserves():
    """the spliced walk writes its last run at nops == cig_cap - 1: with an intron too dear to open, the one-piece checker's rows"""
    import ends_edges as E
    from ciri_long_amd import ssw_wrap
    refs, queries, _ = E.max_runs_rows(E.HOST_GEOM)
    ma, mi, go, ge = E.MAX_RUNS_SCORING
    got = ssw_wrap.align_pairs_spliced(refs, queries, mode='global', strand='+', match=ma, mismatch=mi, gap_open=go, gap_extend=ge, intron_open=1000,
                                       noncanonical=0, report_cigar=True)
    E.check_max_runs(got, E.HOST_GEOM)


def test_a_short_gap_is_a_deletion_and_a_long_one_an_intron_in_the_same_pair():
    rng = chk.rng_for('gpu spliced mixed')
    refs, queries = [], []
    for _ in range(8):
        e1, e2, e3 = (chk.random_seq(rng, 25) for _ in range(3))
        refs.append(chk.random_seq(rng, 7) + e1 + 'CAT' + e2 + _intron(rng, 200) + e3 + chk.random_seq(rng, 6)); queries.append(e1 + e2 + e3)
    wants = _check(refs, queries, 'semiglobal')
    for w in wants:      # where the neighbouring letters repeat, a run may stand a letter to the left
        assert [o for o, _ in w['cigar']] == list('MDMNM') and w['cigar'][1][1] == 3 and w['cigar'][3][1] == 200 and w['score'] == 150 - 5 - 12, w['cigar']
    _check(refs, queries, 'global')
    _check([revcomp(r) for r in refs], [revcomp(q) for q in queries], 'semiglobal', strands=[-1] * 8)


def test_n_letters_in_a_splice_dinucleotide_cost_other_and_a_gc_donor_can_be_cheaper():
    rng = chk.rng_for('gpu spliced sites')
    e1, e2 = chk.random_seq(rng, 25), chk.random_seq(rng, 25)
    body = chk.random_seq(rng, 80, 'ACT')
    refs = ['TTA' + e1 + d + body + a + e2 + 'CCA' for d, a in (('GT', 'AG'), ('NT', 'AG'), ('GN', 'AG'), ('GT', 'NG'), ('GT', 'AN'), ('GC', 'AG'), ('GC', 'AC'))]
    queries = [e1 + e2] * len(refs)
    wants = _check(refs, queries, 'semiglobal')
    assert [w['score'] for w in wants] == [100 - 12, 100 - 18, 100 - 18, 100 - 18, 100 - 18, 100 - 18, 100 - 24]
    gc = dict(DEFAULT, donor={'GC': 2}, acceptor={'AC': 3})
    wants = _check(refs, queries, 'semiglobal', gc)
    assert [w['score'] for w in wants][-2:] == [100 - 14, 100 - 17]
    _check([revcomp(r) for r in refs], [revcomp(q) for q in queries], 'semiglobal', gc, strands=[-1] * len(refs))


def _random_batch(rng, count, max_m=130, max_n=1100):
    refs, queries, strands = [], [], []
    for k in range(count):
        n = rng.choice((1, 2, 7, 8, 9, 63, 64, 65, 511, 512, 513, 1024, 1025, max_n)) if k % 4 == 0 else rng.randint(1, max_n)
        rs = chk.random_seq(rng, n, 'ACGTN' if k % 7 == 0 else 'ACGT')
        if k % 3 and n >= 12:      # a mutated spliced copy: up to three stretches of the reference
            cuts = sorted(rng.sample(range(n + 1), rng.choice((2, 4, 6))))
            qs = ''.join(rs[a:min(b, a + max_m // 3)] for a, b in zip(cuts[::2], cuts[1::2])).replace('N', 'A')
            qs = chk.mutate(rng, qs, 0.1)[:max_m] or 'C'
        else:
            qs = chk.random_seq(rng, rng.choice((1, 63, 64, 65, max_m)) if k % 2 else rng.randint(1, max_m))
        s = 1 if k % 2 else -1
        if s < 0:
            rs, qs = revcomp(rs), revcomp(qs)
        refs.append(rs); queries.append(qs); strands.append(s)
    return refs, queries, strands


def test_a_random_batch_of_200_pairs():
    refs, queries, strands = _random_batch(chk.rng_for('gpu spliced batch'), 200)
    wants = _check(refs, queries, 'semiglobal', strands=strands)
    assert sum('N' in chk.cigar_text(w['cigar']) for w in wants) >= 40


@pytest.mark.parametrize('mode', MODES)
def test_every_mode_on_random_pairs_score_only_and_with_cigars(mode):
    refs, queries, strands = _random_batch(chk.rng_for('gpu spliced modes', mode), 40, max_n=700)
    _check(refs, queries, mode, strands=strands)
    _check(refs[:12], queries[:12], mode, CHEAP, strands=strands[:12])


def test_empty_sides_and_single_letters():
    refs = ['', 'GT' + 'ACT' * 10 + 'AG', '', 'A', 'ACGTACGT', 'G', 'GTAG']
    queries = ['ACGT' * 10, '', '', 'A', 'C', 'ACGTACGT', '']
    for mode in MODES:
        for strand in (1, -1):
            wants = _check(refs, queries, mode, strands=[strand] * len(refs))
            if mode == 'global':
                assert wants[0]['cigar'] == [('I', 40)]
                assert (wants[1]['score'], wants[1]['cigar']) == ((-12, [('N', 34)]) if strand > 0 else (-24, [('N', 34)]))
                assert wants[6]['cigar'] == [('D', 4)]


def test_shares_a_byte_per_cell_two_runs_and_the_capacity_refusal():
    from ciri_long_amd import hip
    rng = chk.rng_for('gpu spliced capacity')
    refs = [chk.random_seq(rng, n) for n in (600, 90, 300, 600, 40)]
    queries = [chk.mutate(rng, r[10:60] + r[-40:], 0.1) for r in refs]
    mat, cmat = hip.score_matrix(2, 2), chk.dna_matrix(2, 2)
    costs = chk.make_costs(**DEFAULT)
    sp = hip.splice_of('test', 12, 6)
    ctx = _ctx()
    qd, qo = hip.pack(queries); rd, ro = hip.pack(refs)
    want = [chk.as_tuple(chk.align(chk.encode(q), chk.encode(r), cmat, costs, 'semiglobal')) for q, r in zip(queries, refs)]
    one = ctx.ends_plan(qd, qo, rd, ro, mat, 3, 1, mode='semiglobal')
    two = ctx.ends_plan(qd, qo, rd, ro, mat, 3, 1, mode='semiglobal', splice=sp)
    try:
        i1, i2 = one.info(), two.info()
        assert 2 * i1['max_pair_bytes'] - 16 <= i2['max_pair_bytes'] <= 2 * i1['max_pair_bytes']      # a byte per cell for half a byte, rounded up to 16
        cells = max(len(q) * 8 * ((len(r) + 7) // 8) for q, r in zip(queries, refs))
        assert cells <= i2['max_pair_bytes'] < cells + 16
        assert i1['shares'] == i2['shares'] == 1 and i2['kernel_pairs'] == 5
        two.run()
        assert _hip_rows(*two.fetch()) == want
    finally:
        one.close(); two.close()
    with pytest.raises(hip.ClhError, match=r'alone needs \d+ bytes of workspace .* workspace_bytes is %d' % i1['max_pair_bytes']):
        ctx.ends_plan(qd, qo, rd, ro, mat, 3, 1, mode='semiglobal', workspace_bytes=i1['max_pair_bytes'], splice=sp)
    cut = ctx.ends_plan(qd, qo, rd, ro, mat, 3, 1, mode='semiglobal', workspace_bytes=i2['max_pair_bytes'], splice=sp)
    try:
        info = cut.info()
        assert info['shares'] >= 3 and info['workspace_bytes'] == i2['max_pair_bytes']
        cut.run()
        first = _hip_rows(*cut.fetch())
        cut.run()
        assert first == _hip_rows(*cut.fetch()) == want
    finally:
        cut.close()


def _abi(mat, n_mat, sp, strand=None, refs=('ACGTACGT',), queries=('ACGT',), go=3, ge=1, workspace=0):
    """clh_ends_batch_spliced itself -> (return code, message)"""
    from ciri_long_amd import hip
    L = hip.lib()
    qd, qo = hip.pack(list(queries)); rd, ro = hip.pack(list(refs))
    mat = np.ascontiguousarray(mat, dtype=np.int8)
    opts = hip.EndsOpts(hip.ENDS_MODES['semiglobal'], mat.ctypes.data, n_mat, go, ge, 1, workspace)
    rows = np.zeros(len(refs), dtype=hip.ENDS_DTYPE)
    cig = np.zeros(64, dtype=np.uint32)
    used = C.c_int64(0)
    st = np.ascontiguousarray(strand, dtype=np.int8) if strand is not None else None
    rc = L.clh_ends_batch_spliced(_ctx()._h, len(refs), qd.ctypes.data, qo.ctypes.data, rd.ctypes.data, ro.ctypes.data, C.byref(opts),
                                  C.byref(sp) if sp is not None else None, st.ctypes.data if st is not None else None, rows.ctypes.data, cig.ctypes.data, 64,
                                  C.byref(used))
    return rc, hip.last_error(), rows, cig[:used.value]


def test_refusals_and_their_codes():
    from ciri_long_amd import hip, ssw_wrap
    E_ARG, E_UNSUPPORTED, E_CAPACITY = -2, -3, -4
    sp = hip.splice_of('test', 12, 6)
    dna = hip.score_matrix(2, 2)
    rc, _, rows, cig = _abi(dna, 5, sp)
    assert rc == 0 and int(rows[0]['score']) == 8 and list(cig) == [(4 << 4) | 0]
    # a matrix that is not match / mismatch, and another alphabet
    odd = dna.copy(); odd[1] = 1
    assert _abi(odd, 5, sp)[0] == E_UNSUPPORTED and 'match / mismatch matrix alone' in hip.last_error()
    assert _abi(np.ones(16, dtype=np.int8), 4, sp)[0] == E_UNSUPPORTED
    # two-piece gap costs together with introns
    with pytest.raises(hip.ClhError, match='CLH_E_UNSUPPORTED: two-piece gap costs together with introns'):
        _ctx().ends_plan(hip.encode('A'), [0, 1], hip.encode('A'), [0, 1], dna, 3, 1, gap_open2=24, gap_extend2=1, splice=sp)
    # arguments
    assert _abi(dna, 5, None)[0] == E_ARG
    assert _abi(dna, 5, sp, strand=[0])[0] == E_ARG and 'strand must be +1 or -1' in hip.last_error()
    neg = hip.splice_of('test', 12, 6); neg.acceptor[5] = -1
    assert _abi(dna, 5, neg)[0] == E_ARG and 'must not be negative' in hip.last_error()
    assert _abi(dna, 5, sp, go=1, ge=2)[0] == E_UNSUPPORTED
    # the range bound takes io + dmax + amax: (4 + 4) 2^27 = 2^30 is the bound itself
    big = 1 << 27
    with pytest.raises(hip.ClhError, match=r'pair 1: \(m \+ n\) \* max\(\|s\|, gap_open, gap_extend, intron_open \+ dmax \+ amax\) = 8 \* %d reaches 2\^30' % big):
        ssw_wrap.align_pairs_spliced(['A', 'ACGT'], ['A', 'ACGT'], intron_open=big - 12, noncanonical=6)
    assert _abi(dna, 5, hip.splice_of('test', big - 12, 6), refs=['ACGT'], queries=['ACGT'])[0] == E_ARG
    for mode in MODES:      # one below the bound: (4 + 3) (2^27 - 1) < 2^30
        _check(['A', 'ACGT', 'GTAG'], ['A', 'ACG', 'AG'], mode, dict(go=3, ge=1, io=big - 13, noncanonical=6))
    # one pair above workspace_bytes
    rc, msg, _, _ = _abi(dna, 5, sp, refs=['ACGT' * 50], queries=['ACGT' * 10], workspace=1024)
    assert rc == E_CAPACITY and 'alone needs 8000 bytes of workspace' in msg


@pytest.mark.parametrize('mode', MODES)
def test_an_intron_too_dear_to_win_gives_the_rows_and_cigars_of_align_pairs_ends(mode):
    from ciri_long_amd import ssw_wrap
    refs, queries, _ = _random_batch(chk.rng_for('gpu spliced dear', mode), 40, max_n=700)
    refs += ['', 'ACGT' * 6, 'GT' + 'ACT' * 20 + 'AG']; queries += ['ACGTAC', '', '']
    io = 3 + max(len(r) for r in refs) * 1 + 1                     # io > go + n ge: no run is cheaper as an intron
    old = ssw_wrap.align_pairs_ends(refs, queries, mode=mode, report_cigar=True)
    for strand in ('+', '-'):
        new = ssw_wrap.align_pairs_spliced(refs, queries, mode=mode, strand=strand, intron_open=io, noncanonical=0, report_cigar=True)
        for k, (a, b) in enumerate(zip(old, new)):
            assert (a.score, a.ref_begin, a.ref_end, a.query_begin, a.query_end, a.cigar_string) == \
                   (b.score, b.ref_begin, b.ref_end, b.query_begin, b.query_end, b.cigar_string), (k, mode, strand)
