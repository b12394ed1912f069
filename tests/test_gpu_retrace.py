"""K1g's recompute route to the CIGARs (traceback='recompute': kept chunk columns, one chunk's decisions computed again at a time, a walk
resumed chunk after chunk; csrc/ssw_ends.hip, csrc/ssw_pairs.h) on the GPU.  Every case runs through traceback='recompute' and is
held two ways: to the same call with traceback='stored' on the same device, rows and CIGAR ops equal as arrays, and to the model's
checker (tests/ends_check.py, anchored_check.py, twopiece_check.py, spliced_check.py), field by field with every CIGAR rescored on its
own.  The shapes are the smallest with one, two, three and five chunks of 512 columns: m <= 130, n <= 2 400."""
import numpy as np
import pytest

import anchored_check as ac
import ends_check as ec
import spliced_check as sc
import twopiece_check as tc

pytestmark = pytest.mark.gpu

MODES = ('global', 'semiglobal', 'overlap', 'prefix', 'extend')
MODELS = ('one', 'two', 'spliced')
ONE = dict(match=2, mismatch=2, go=3, ge=1)
TWO = dict(match=2, mismatch=4, go=4, ge=2, go2=24, ge2=1)          # ssw_wrap.LONG_READ_GAPS
SPL = dict(go=3, ge=1, io=12, noncanonical=6)


def _ctx():
    from ciri_long_amd import hip
    return hip.default_context()


def revcomp(s):
    return ''.join({'A': 'T', 'C': 'G', 'G': 'C', 'T': 'A', 'N': 'N'}[c] for c in reversed(s))


def _plan_args(model, queries, refs, strands=None, matrix=None, alphabet=None, go=None, ge=None):
    """-> (positional arguments of Context.ends_plan / ends_batch up to gap_extend, keywords of the model)"""
    from ciri_long_amd import hip, ssw_wrap
    if matrix is not None:
        enc = lambda s: ssw_wrap.encode_alphabet(s, alphabet)
        mat = np.ascontiguousarray(matrix, dtype=np.int8)
    else:
        enc = hip.encode
        mat = hip.score_matrix(*((TWO['match'], TWO['mismatch']) if model == 'two' else (2, 2)))
    qd, qo = hip.pack([enc(q) for q in queries]); rd, ro = hip.pack([enc(r) for r in refs])
    kw = {}
    if model == 'two':
        go, ge = TWO['go'], TWO['ge']
        kw = dict(gap_open2=TWO['go2'], gap_extend2=TWO['ge2'])
    elif model == 'spliced':
        go, ge = SPL['go'], SPL['ge']
        kw = dict(splice=hip.splice_of('test', SPL['io'], SPL['noncanonical'], None, None),
                  strand=np.array(strands if strands is not None else [1] * len(refs), dtype=np.int8))
    elif go is None:
        go, ge = ONE['go'], ONE['ge']
    return (qd, qo, rd, ro, mat, go, ge), kw


def _rows(rows, cig):
    return [(int(r['score']), int(r['ref_begin']), int(r['ref_end']), int(r['query_begin']), int(r['query_end']),
             ec.cigar_text([('MIDN'[int(c) & 15], int(c) >> 4) for c in cig[int(r['cigar_off']):int(r['cigar_off']) + int(r['cigar_len'])]]))
            for r in rows]


def _want(model, q, r, mode, strand=1, matrix=None, alphabet=None, go=None, ge=None):
    """the checker's result of one pair, its CIGAR rescored"""
    if matrix is not None:
        qe, re_, mat = ec.encode(q, alphabet), ec.encode(r, alphabet), np.asarray(matrix, dtype=np.int64)
    else:
        qe, re_ = ec.encode(q), ec.encode(r)
        mat = ec.dna_matrix(TWO['match'], TWO['mismatch']) if model == 'two' else ec.dna_matrix(2, 2)
    if model == 'one':
        go, ge = (ONE['go'], ONE['ge']) if go is None else (go, ge)
        chk = ec if mode in ec.MODES else ac
        want = chk.align(qe, re_, mat, go, ge, mode)
        chk.check_cigar(want, qe, re_, mat, go, ge, mode)
    elif model == 'two':
        costs = (TWO['go'], TWO['ge'], TWO['go2'], TWO['ge2'])
        want = tc.align(qe, re_, mat, costs, mode)
        tc.check_cigar(want, qe, re_, mat, costs, mode)
    else:
        costs = sc.make_costs(**SPL)
        want = sc.align(qe, re_, mat, costs, mode, strand)
        sc.check_cigar(want, qe, re_, mat, costs, mode, strand)
    return ec.as_tuple(want)


def _both_routes(model, queries, refs, mode, strands=None, **scoring):
    """the pairs through both routes: rows and ops equal as arrays -> the recompute route's rows as tuples"""
    args, kw = _plan_args(model, queries, refs, strands, **scoring)
    ctx = _ctx()
    srows, scig = ctx.ends_batch(*args, mode=mode, traceback='stored', **kw)
    rrows, rcig = ctx.ends_batch(*args, mode=mode, traceback='recompute', **kw)
    assert srows.tobytes() == rrows.tobytes() and np.array_equal(scig, rcig), (model, mode)
    return _rows(rrows, rcig)


def _check(model, queries, refs, mode, strands=None, **scoring):
    got = _both_routes(model, queries, refs, mode, strands, **scoring)
    strands = strands if strands is not None else [1] * len(refs)
    for k, (q, r, s) in enumerate(zip(queries, refs, strands)):
        assert got[k] == _want(model, q, r, mode, s, **scoring), (model, mode, k, len(q), len(r))
    return got


def _query(rng, ref, a, m):
    """a 10 % mutated slice of the reference from letter a, of exactly m letters"""
    q = ec.mutate(rng, ref[a:a + m + 8], 0.1)[:m]
    return q + ec.random_seq(rng, m - len(q))


def _geometry(rng):
    """(query, reference): m and n at the row-block and chunk edges, the query placed in chunk 0, a middle chunk, the last chunk and
    astride columns 480..560"""
    out = []
    for n in (512, 513, 520, 1024, 1025, 1537, 2049):
        ref = ec.random_seq(rng, n)
        nch = (n + 511) // 512
        for m in (1, 63, 64, 65, 129):
            places = {min(5, n - m), min(512 * (nch // 2) + 100, n - m), max(0, n - m - 3), max(0, min(520 - m // 2, n - m))}
            out.extend((_query(rng, ref, a, m), ref) for a in sorted(places))
    return out


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('model', MODELS)
def test_rows_and_chunks_at_their_edges_with_the_end_cell_in_every_chunk(model, mode):
    pairs = _geometry(ec.rng_for('gpu retrace geometry', model, mode))
    assert len(pairs) > 100
    strands = [1 if k % 3 else -1 for k in range(len(pairs))] if model == 'spliced' else None
    _check(model, [p[0] for p in pairs], [p[1] for p in pairs], mode, strands)


def _op_over_edge(cigar_text, ref_begin, op, edge=512):
    """the one run of `op` that holds both the 1-based columns edge and edge + 1 -> its length; the CIGAR has no other run of op"""
    ops = ec.parse_cigar(cigar_text)
    assert [o for o, _ in ops].count(op) == 1, cigar_text
    j = ref_begin                                              # reference letters consumed
    for o, k in ops:
        if o == op:
            assert j < edge and j + k > edge, (cigar_text, ref_begin)
            return k
        j += k if o in 'MDN' else 0


def test_the_walk_crosses_column_512_on_the_diagonal_in_a_deletion_and_beside_an_insertion():
    rng = ec.rng_for('gpu retrace states')
    ref = ec.random_seq(rng, 700)
    # the inserted letters begin with none of the two reference letters behind the edges and end with none of the two in front of them, so
    # the insertion can stand nowhere else at the same score
    ins = [x for x in 'ACGT' if x not in ref[512:514]][0] + 'ACGTTG' + [x for x in 'ACGT' if x not in ref[511:513]][0]
    queries = [ref[480:560],                                   # the diagonal
               ref[440:500] + ref[530:590],                    # a deletion of columns 501..530
               ref[470:512] + ins + ref[512:560],              # an insertion run standing on column 512
               ref[470:513] + ins + ref[513:560]]              # ... and on column 513
    got = _check('one', queries, [ref] * 4, 'semiglobal')
    assert got[0][5] == '80M' and (got[0][1], got[0][2]) == (480, 559)
    assert _op_over_edge(got[0][5], got[0][1], 'M') == 80
    assert _op_over_edge(got[1][5], got[1][1], 'D') == 30
    for k in (2, 3):
        ops = ec.parse_cigar(got[k][5])
        assert [o for o, _ in ops] == ['M', 'I', 'M'] and ops[1][1] == len(ins), got[k]
    assert got[2][1] + ec.parse_cigar(got[2][5])[0][1] == 512 and got[3][1] + ec.parse_cigar(got[3][5])[0][1] == 513


def test_a_second_piece_run_of_600_letters_that_covers_a_whole_chunk_is_one_op():
    # global: the reference is consumed whatever it costs, and the flanks (G / T) match nothing of the fill (A / C)
    rng = ec.rng_for('gpu retrace E2')
    a, b = ec.random_seq(rng, 65, 'GT'), ec.random_seq(rng, 65, 'GT')
    ref = ec.random_seq(rng, 415, 'AC') + a + ec.random_seq(rng, 600, 'AC') + b
    got = _check('two', [a + b], [ref], 'global')
    assert got[0][5] == '415D65M600D65M'                      # columns 481..1080: chunk 1 (513..1024) lies inside the run


def _intron(rng, length):
    return 'GT' + ec.random_seq(rng, length - 4, 'ACT') + 'AG'


def _spliced_pair(rng, first, length, strand, ins_before='', ins_after=''):
    """two exons of 30 letters around an intron whose first letter is the 1-based column `first` of the reference as the device
    reads it, on either strand -> (query, reference)"""
    letters = 'ACT' if ins_before or ins_after else 'ACGT'      # beside an insertion of G: no exon letter it could be taken for
    e1, e2 = ec.random_seq(rng, 30, letters), ec.random_seq(rng, 30, letters)
    if strand > 0:
        head, tail = ec.random_seq(rng, first - 31, 'AT'), ec.random_seq(rng, 7, 'AT')
    else:                                                      # the reverse complement puts the tail in front
        head, tail = ec.random_seq(rng, 7, 'AT'), ec.random_seq(rng, first - 31, 'AT')
    q, r = e1 + ins_before + ins_after + e2, head + e1 + _intron(rng, length) + e2 + tail
    return (q, r) if strand > 0 else (revcomp(q), revcomp(r))


@pytest.mark.parametrize('strand', (1, -1))
def test_an_intron_over_two_whole_chunks_with_its_ends_at_the_chunk_edges_is_one_op(strand):
    # 1 300 letters: from column 511, 512, 513, 1024 or 1025 on, and up to column 1535, 1536, 1537, 2048 or 2049 (an intron of that
    # length cannot end at the first edges, nor begin at the last ones inside 2 400 columns)
    rng = ec.rng_for('gpu retrace introns', strand)
    pairs = [_spliced_pair(rng, first, 1300, strand) for first in (511, 512, 513, 1024, 1025)]
    pairs += [_spliced_pair(rng, last - 1299, 1300, strand) for last in (1535, 1536, 1537, 2048, 2049)]
    assert max(len(r) for _, r in pairs) <= 2400
    got = _check('spliced', [p[0] for p in pairs], [p[1] for p in pairs], 'semiglobal', [strand] * len(pairs))
    firsts = (511, 512, 513, 1024, 1025, 1535 - 1299, 1536 - 1299, 1537 - 1299, 2048 - 1299, 2049 - 1299)
    for g, first in zip(got, firsts):
        assert g[5] == '30M1300N30M' and g[1] + 30 + 1 == first and g[0] == 120 - 12, (g, first)
    # and an intron of 400 letters that ends at the first edges themselves
    lasts = (511, 512, 513, 1024, 1025)
    pairs = [_spliced_pair(rng, last - 399, 400, strand) for last in lasts]
    got = _check('spliced', [p[0] for p in pairs], [p[1] for p in pairs], 'semiglobal', [strand] * len(pairs))
    for g, last in zip(got, lasts):
        assert g[5] == '30M400N30M' and g[1] + 30 + 400 == last and g[0] == 120 - 12, (g, last)


@pytest.mark.parametrize('strand', (1, -1))
def test_an_insertion_beside_an_intron_that_opens_or_closes_at_a_chunk_edge(strand):
    # Three query letters between the exons: among the equal alignments the walk takes N before F, so the insertion stands in front
    # of the intron.  The intron's first letter at column 513 (1025): the walk leaves the N run at column 512 (1024), is suspended in
    # state T and finds F in the next round's tile.  Its last letter at column 512 (1024): the N run begins on a chunk's last column.
    rng = ec.rng_for('gpu retrace state T', strand)
    pairs = [_spliced_pair(rng, 513, 700, strand, ins_before='GGG'), _spliced_pair(rng, 1025, 700, strand, ins_before='GGG'),
             _spliced_pair(rng, 512 - 399, 400, strand, ins_after='GGG'), _spliced_pair(rng, 1024 - 699, 700, strand, ins_after='GGG')]
    got = _check('spliced', [p[0] for p in pairs], [p[1] for p in pairs], 'semiglobal', [strand] * len(pairs))
    for g in got:
        ops = [o for o, _ in ec.parse_cigar(g[5])]
        assert ''.join(ops) == 'MINM' and g[0] == 120 - 12 - 5, g


@pytest.mark.parametrize('model', MODELS)
def test_row_0_is_reached_outside_chunk_0(model):
    rng = ec.rng_for('gpu retrace row 0', model)
    ref = ec.random_seq(rng, 1300)
    got = _check(model, [ref[1100:1140]], [ref], 'global')
    ops = ec.parse_cigar(got[0][5])
    assert ops[0] == ('N' if model == 'spliced' else 'D', 1100) and ops[1][0] == 'M', got[0]      # 12 + 6 + 6 against 3 + 1 099
    semi = _check(model, [ref[1100:1140], 'GGGGGGGGGG' + ref[0:40].replace('G', 'A')], [ref, ref.replace('G', 'A')], 'semiglobal')
    assert semi[0][5] == '40M' and semi[0][1] == 1100
    assert semi[1][1] == 0 and ec.parse_cigar(semi[1][5])[0][0] == 'I', semi[1]                      # column 0 with query letters left


def test_capacity_between_the_two_routes_and_one_pair_a_share():
    from ciri_long_amd import hip
    rng = ec.rng_for('gpu retrace capacity')
    refs = [ec.random_seq(rng, 1600) for _ in range(4)]
    queries = [_query(rng, r, 1000 + 40 * k, 40) for k, r in enumerate(refs)]
    args, kw = _plan_args('one', queries, refs)
    ctx = _ctx()
    need = {}
    for route in ('stored', 'recompute'):
        plan = ctx.ends_plan(*args, mode='global', traceback=route, **kw)
        try:
            info = plan.info()
            need[route] = info['max_pair_bytes']
            assert info['traceback'] == route and info['shares'] == 1 and info['workspace_bytes'] == 4 * need[route]
        finally:
            plan.close()
    # 4 x 40 x (64 x 3 + 8) bytes against 3 kept columns of 2 x 64 int32, a plane of 4 x 40 x 64 bytes and the record
    assert need['stored'] == 4 * 40 * (64 * 3 + 8) and need['recompute'] == (3 * 2 * 64 * 4 + 4 * 40 * 64 + 48 + 15) // 16 * 16
    between = (need['stored'] + need['recompute']) // 2
    with pytest.raises(hip.ClhError, match='alone needs %d bytes of workspace' % need['stored']):
        ctx.ends_plan(*args, mode='global', traceback='stored', workspace_bytes=between, **kw)
    want = [_want('one', q, r, 'global') for q, r in zip(queries, refs)]
    assert _rows(*ctx.ends_batch(*args, mode='global', traceback='recompute', workspace_bytes=between, **kw)) == want
    plan = ctx.ends_plan(*args, mode='global', traceback='recompute', workspace_bytes=need['recompute'], **kw)
    try:
        info = plan.info()
        assert info['shares'] == 4 and info['workspace_bytes'] == need['recompute']
        plan.run()
        assert _rows(*plan.fetch()) == want
    finally:
        plan.close()
    with pytest.raises(hip.ClhError, match='alone needs %d bytes of workspace' % need['recompute']):
        ctx.ends_plan(*args, mode='global', traceback='recompute', workspace_bytes=need['recompute'] - 1, **kw)


@pytest.mark.parametrize('model', MODELS)
@pytest.mark.parametrize('mode', ('extend', 'global'))
def test_pairs_that_finish_in_different_rounds_in_one_plan_run_twice(model, mode):
    rng = ec.rng_for('gpu retrace mixture', model, mode)
    long_ref = ec.random_seq(rng, 2100)
    refs = [ec.random_seq(rng, 300), long_ref, '', ec.random_seq(rng, 50), 'CCCCCCCC', long_ref, ec.random_seq(rng, 700)]
    queries = [_query(rng, refs[0], 0, 90), _query(rng, long_ref, 0, 120), 'ACGT', '', 'AAAA', _query(rng, long_ref, 1990, 100), _query(rng, refs[6], 0, 64)]
    args, kw = _plan_args(model, queries, refs)
    ctx = _ctx()
    plan = ctx.ends_plan(*args, mode=mode, traceback='recompute', **kw)
    try:
        assert plan.info()['empty_pairs'] == 2
        plan.run()
        first = plan.fetch()
        plan.run()
        second = plan.fetch()
    finally:
        plan.close()
    assert first[0].tobytes() == second[0].tobytes() and np.array_equal(first[1], second[1])
    stored = ctx.ends_batch(*args, mode=mode, traceback='stored', **kw)
    assert first[0].tobytes() == stored[0].tobytes() and np.array_equal(first[1], stored[1])
    got = _rows(*first)
    for k, (q, r) in enumerate(zip(queries, refs)):
        if q and r:
            assert got[k] == _want(model, q, r, mode), (model, mode, k)
    if mode == 'extend':
        assert got[4] == (0, 0, -1, 0, -1, '')               # the empty result: no round is needed


def test_blosum62_global_over_two_chunks():
    from ciri_long_amd import ssw_wrap
    rng = ec.rng_for('gpu retrace blosum')
    letters = ssw_wrap.BLOSUM62_ALPHABET[:20]
    refs = [ec.random_seq(rng, 700, letters) for _ in range(3)]
    queries = [ec.mutate(rng, r[300 * k:300 * k + 100], 0.15, letters) for k, r in enumerate(refs)]
    _check('one', queries, refs, 'global', matrix=ssw_wrap.BLOSUM62, alphabet=ssw_wrap.BLOSUM62_ALPHABET, go=11, ge=1)


def test_the_wrappers_pass_the_route_on_and_refuse_what_is_not_one():
    from ciri_long_amd import ssw_wrap
    rng = ec.rng_for('gpu retrace wrappers')
    ref = ec.random_seq(rng, 1200)
    q = _query(rng, ref, 600, 80)
    for fn, kw in ((ssw_wrap.align_pairs_ends, dict(mode='semiglobal')), (ssw_wrap.align_pairs_spliced, dict(mode='semiglobal'))):
        a = fn([ref], [q], report_cigar=True, traceback='stored', **kw)[0]
        b = fn([ref], [q], report_cigar=True, traceback='recompute', **kw)[0]
        assert (a.score, a.ref_begin, a.ref_end, a.cigar_string) == (b.score, b.ref_begin, b.ref_end, b.cigar_string) and b.cigar_string
        with pytest.raises(ValueError, match='traceback'):
            fn([ref], [q], traceback='kept', **kw)
    a = ssw_wrap.extend_anchors([ref], [q], [(640, 40)], report_cigar=True)[0]
    b = ssw_wrap.extend_anchors([ref], [q], [(640, 40)], report_cigar=True, traceback='recompute')[0]
    assert (a.score, a.ref_begin, a.ref_end, a.query_begin, a.query_end, a.cigar_string) == (b.score, b.ref_begin, b.ref_end, b.query_begin, b.query_end, b.cigar_string)
    with pytest.raises(ValueError, match='band=None'):
        ssw_wrap.extend_anchors([ref], [q], [(640, 40)], band=16, traceback='recompute')
    with pytest.raises(ValueError, match='traceback'):
        ssw_wrap.extend_anchors([ref], [q], [(640, 40)], traceback='both')
    with pytest.raises(ValueError, match='traceback'):
        _ctx().ends_plan(*_plan_args('one', [q], [ref])[0], traceback='none')
