"""Alignments over substitution matrices of 6..32 letters on the GPU (K1a, csrc/ssw_alpha.hip) at the edges of
tests/ssw_alphabet_edges.py, bit-exact as whole result dicts with CIGARs and status bits against the reference's answers in
tests/golden/ssw_alphabet_edges_golden.json.gz; more global-form alignments than the form has workgroups and a batch whose tracebacks
outgrow the plan's pool share against the CPU oracle.  Every set first asserts, from plan.segments(), which K1a class (-10..-14, one per
read-length bucket) takes each case, so that a later routing change cannot silently stop testing an edge.  Entry points:
Context.ssw_batch, a plan run twice, the legacy ssw_init / ssw_align of libclh.so, ssw_wrap.align_pairs_matrix."""
import gzip
import json
import os
from collections import Counter

import numpy as np
import pytest

import oracle_lib
import ssw_alphabet_edges as edges
from oracle_lib import mask_len, oracle_align
from test_gpu_ssw_alphabet import _legacy, as_dict

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
K1A, GLOBAL_FORM = -10, -14


@pytest.fixture(scope='module')
def ctx():
    from ciri_long_amd import hip
    return hip.Context(0)


def _golden():
    with gzip.open(os.path.join(HERE, 'golden', edges.GOLDEN_NAME), 'rt') as f:
        return json.load(f)['cases']


def bucket_class(L):
    """the K1a class of a read of L letters (clh_api.hip alpha_class_for)"""
    for b, rows in enumerate(edges.ALPHA_ROWS):
        if L <= rows:
            return K1A - b
    return GLOBAL_FORM


def stated_trunc(w):
    """the condition under which K1a states CLH_ST_CIGAR_TRUNC: an aligned read over 5 121 rows with a band the big launch's ring cannot hold"""
    la, ra = w['query_end'] - w['query_begin'] + 1, w['ref_end'] - w['ref_begin'] + 1
    return la + 1 > edges.BIG_WS and abs(ra - la) + 1 + 3 > edges.BIG_RING


def groups(key):
    """the cases of a golden set with their answers, grouped into batches of one option set: [(mat, kw, [(ref, read, maskl, want)])]"""
    out = {}
    for c, w in zip(edges.all_cases()[key], _golden()[key]):
        assert edges.case_crc(c) == w['crc'], key
        (ref, read), kw = edges.call_args(c)
        maskl = kw.pop('maskl', mask_len(len(read)))
        m = kw.pop('mat')
        gk = (tuple(int(x) for x in m), tuple(sorted(kw.items())))
        out.setdefault(gk, (m, kw, []))[2].append((ref, read, maskl, w['want']))
    return list(out.values())


def assert_classes(ctx, refs, reads, mat, kw, masks):
    from ciri_long_amd import hip
    _rd, ro = hip.pack(reads); _fd, fo = hip.pack(refs)
    plan = ctx.plan(ro, fo, mat, kw['gap_open'], kw['gap_extend'], flag=kw['flag'], score_size=kw['score_size'],
                    mask_len=np.asarray(masks, dtype=np.int32))
    got = Counter()
    for rv, n, _a, _b in plan.segments():
        got[rv] += n
    plan.close()
    want = Counter(bucket_class(len(q)) for q in reads)
    assert got == want, (dict(got), dict(want))
    return got


def check_rows(rows, cig, reads, mat, kw, wants, tag):
    """whole result dicts against the answers; the status bits: WORD exactly where the 8-bit pass overflowed (or score_size 1), NULL
    exactly where the reference returns NULL, no traceback error, CIGAR_TRUNC only under the stated condition"""
    from ciri_long_amd import hip
    bias = -min(0, int(np.min(mat)))
    for k, w in enumerate(wants):
        r = rows[k]
        st = int(r['status'])
        where = (tag, k, len(reads[k]))
        assert not st & hip.ST_TRACE_ERR, where
        assert bool(st & hip.ST_NULL) == (w is None), where
        if w is None:
            continue
        word = kw['score_size'] == 1 or w['score'] + bias >= 255
        assert bool(st & hip.ST_WORD) == word, where
        if w['cigar'] and stated_trunc(w):
            assert st & hip.ST_CIGAR_TRUNC, where
            got = (int(r['score1']), int(r['score2']), int(r['ref_begin1']), int(r['ref_end1']), int(r['read_begin1']), int(r['read_end1']),
                   int(r['ref_end2']))
            assert got == (w['score'], w['score2'], w['ref_begin'], w['ref_end'], w['query_begin'], w['query_end'], w['ref_end2']), where
            continue
        assert not st & hip.ST_CIGAR_TRUNC, where
        assert as_dict(r, cig, len(reads[k])) == w, where


def run_golden_set(ctx, key):
    from ciri_long_amd import hip
    seen = Counter()
    for mat, kw, items in groups(key):
        refs = [i[0] for i in items]; reads = [i[1] for i in items]; masks = [i[2] for i in items]; wants = [i[3] for i in items]
        seen += assert_classes(ctx, refs, reads, mat, kw, masks)
        rd, ro = hip.pack(reads); fd, fo = hip.pack(refs)
        rows, cig = ctx.ssw_batch(rd, ro, fd, fo, mat, kw['gap_open'], kw['gap_extend'], flag=kw['flag'], score_size=kw['score_size'],
                                  want_score2=True, want_cigar=True, mask_len=np.asarray(masks, dtype=np.int32),
                                  filters=kw['filters'], filterd=kw['filterd'])
        check_rows(rows, cig, reads, mat, kw, wants, key)
    return seen


@pytest.mark.parametrize('key', ['asymmetric', '8-bit threshold', 'gap costs'])
def test_golden_sets(ctx, key):
    run_golden_set(ctx, key)


def test_buckets(ctx):
    seen = run_golden_set(ctx, 'buckets')
    assert set(seen) == {K1A - b for b in range(5)}, seen


def test_ceiling(ctx):
    seen = run_golden_set(ctx, 'ceiling')
    assert {K1A - 1, K1A - 2, GLOBAL_FORM} <= set(seen), seen          # the diagonal-127 reads, BLOSUM62 W-W, the diagonal of 4


def test_traceback_windows(ctx):
    """one batch: classes -11 (bands 509..511, 255 -> 510), -12 (read + reference 6 144 / 6 145) and -13 (longest read 5 300 rows: the big
    launch's 5 122 rows, its ring of 4 096, 10 184 bytes of staged sequence)"""
    seen = run_golden_set(ctx, 'traceback windows')
    assert seen == Counter({K1A - 1: 7, K1A - 2: 2, K1A - 3: 9}), seen
    assert sum(stated_trunc(w['want']) for w in _golden()['traceback windows']) >= 2


def test_plan_runs_twice(ctx):
    """the ceiling (reads below 4 000 letters) and threshold sets through Context.plan: one plan per option set, run twice on a side stream"""
    import torch
    from ciri_long_amd import hip
    ts = torch.cuda.Stream()
    for key in ('ceiling', '8-bit threshold'):
        for mat, kw, items in groups(key):
            items = [i for i in items if len(i[1]) < 4000]
            if not items:
                continue
            refs = [i[0] for i in items]; reads = [i[1] for i in items]; masks = [i[2] for i in items]; wants = [i[3] for i in items]
            rd, ro = hip.pack(reads); fd, fo = hip.pack(refs)
            d_r = torch.from_numpy(rd.view(np.uint8)).cuda(); d_f = torch.from_numpy(fd.view(np.uint8)).cuda()
            torch.cuda.synchronize()
            plan = ctx.plan(ro, fo, mat, kw['gap_open'], kw['gap_extend'], flag=kw['flag'], score_size=kw['score_size'],
                            mask_len=np.asarray(masks, dtype=np.int32))
            assert all(-14 <= rv <= -10 for rv, _c, _a, _b in plan.segments())
            for _ in range(2):
                plan.run(d_r.data_ptr(), d_f.data_ptr(), ts.cuda_stream)
                rows, cig = plan.fetch()
                check_rows(rows, cig, reads, mat, kw, wants, key + ' plan')
            plan.close()


def test_legacy_ssw_align_ceiling_and_threshold(ctx, capfd):
    """ssw_init / ssw_align of libclh.so on saturated and near-ceiling cases and on both sides of the 8-bit threshold (NULL where the
    reference returns NULL)"""
    L = _legacy()
    picked = [(c, w['want']) for c, w in zip(edges.all_cases()['ceiling'], _golden()['ceiling'])
              if w['want']['score'] in (32766, 32767) and len(c[1]) < 1200]
    picked += list(zip(edges.all_cases()['8-bit threshold'], [w['want'] for w in _golden()['8-bit threshold']]))[:48]
    assert any(w is None for _c, w in picked) and any(w and w['score'] == 32767 for _c, w in picked)
    for c, want in picked:
        (ref, read), kw = edges.call_args(c)
        mat = np.ascontiguousarray(kw['mat']); n = int(round(len(mat) ** 0.5))
        q = np.ascontiguousarray(read); r = np.ascontiguousarray(ref)
        prof = L.ssw_init(q.ctypes.data, len(q), mat.ctypes.data, n, kw['score_size'])
        p = L.ssw_align(prof, r.ctypes.data, len(r), kw['gap_open'], kw['gap_extend'], kw['flag'], kw['filters'], kw['filterd'],
                        kw.get('maskl', mask_len(len(q))))
        L.init_destroy(prof)
        if want is None:
            assert not p
            continue
        assert p
        res = p.contents
        cg = [res.cigar[i] for i in range(res.cigarLen)]
        got = dict(score=res.score1, score2=res.score2, ref_begin=res.ref_begin1, ref_end=res.ref_end1, query_begin=res.read_begin1,
                   query_end=res.read_end1, ref_end2=res.ref_end2, cigar=cg,
                   cigar_string=oracle_lib.cigar_to_string(cg, res.read_begin1, res.read_end1, len(q)) if cg else None)
        L.align_destroy(p)
        assert got == want, len(q)
    capfd.readouterr()


def test_align_pairs_matrix_buckets(ctx):
    """the BLOSUM62 cases of the bucket set with reads of 1..8 193 letters (all five classes) through ssw_wrap.align_pairs_matrix"""
    from ciri_long_amd import ssw_wrap
    A = ssw_wrap.BLOSUM62_ALPHABET
    b62 = edges.blosum62()
    pairs = [(c, w['want']) for c, w in zip(edges.all_cases()['buckets'], _golden()['buckets']) if list(c[2]) == b62 and len(c[1]) <= 8193]
    assert {bucket_class(len(c[1])) for c, _w in pairs} == {K1A - b for b in range(5)}
    rs, qs = [], []
    for c, _w in pairs:
        (ref, read), kw = edges.call_args(c)
        assert (kw['gap_open'], kw['gap_extend'], kw['flag'], kw['score_size']) == (11, 1, 1, 2)
        rs.append(''.join(A[x] for x in ref)); qs.append(''.join(A[x] for x in read))
    got = ssw_wrap.align_pairs_matrix(rs, qs, ssw_wrap.BLOSUM62, A, 11, 1, report_secondary=True, report_cigar=True, context=ctx)
    for k, (_c, w) in enumerate(pairs):
        g = got[k]
        assert (g.score, g.ref_begin, g.ref_end, g.query_begin, g.query_end) == \
            (w['score'], w['ref_begin'], w['ref_end'], w['query_begin'], w['query_end']), k
        assert (g.score2, g.ref_end2) == ((w['score2'], w['ref_end2']) if w['score2'] != 0 else (None, None)), k
        assert g.cigar_string == w['cigar_string'], k


def _check_against_oracle(rows, cig, refs, reads, mat, o, e, tag):
    from ciri_long_amd import hip
    check = oracle_lib.ref_align if oracle_lib.have_ref() else oracle_align
    bias = -min(0, int(np.min(mat)))
    for k in range(len(reads)):
        w = check(refs[k], reads[k], gap_open=o, gap_extend=e, flag=1, score_size=2, mat=mat)
        st = int(rows[k]['status'])
        assert not st & (hip.ST_TRACE_ERR | hip.ST_CIGAR_TRUNC | hip.ST_NULL), (tag, k, st)
        assert bool(st & hip.ST_WORD) == (w['score'] + bias >= 255), (tag, k)
        assert as_dict(rows[k], cig, len(reads[k])) == w, (tag, k, len(reads[k]), len(refs[k]))


def test_global_form_more_tasks_than_workgroups(ctx):
    """n_cu * 8 + 100 alignments above 8 192 rows: the persistent workgroups of the global form each take several, reusing their slot"""
    import torch
    from ciri_long_amd import hip
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    refs, reads, mat = edges.global_many(n_cu)
    mat = np.asarray(mat, dtype=np.int8)
    masks = np.asarray([mask_len(len(q)) for q in reads], dtype=np.int32)
    assert len(reads) >= n_cu * 8 + 100
    assert assert_classes(ctx, refs, reads, mat, dict(gap_open=5, gap_extend=1, flag=1, score_size=2), masks) == Counter({GLOBAL_FORM: len(reads)})
    rd, ro = hip.pack(reads); fd, fo = hip.pack(refs)
    rows, cig = ctx.ssw_batch(rd, ro, fd, fo, mat, 5, 1, flag=1, score_size=2, want_score2=True, want_cigar=True, mask_len=masks)
    _check_against_oracle(rows, cig, refs, reads, mat, 5, 1, 'global form')


def test_traceback_pool_pressure(ctx):
    """one ssw_batch of 450 BLOSUM62 pairs whose alignments skip 2 000 reference letters: about 4 MB of traceback bytes each, against a
    plan share of 340 kB and 1 GiB of slack.  Every CIGAR equal to the oracle's, none truncated"""
    from ciri_long_amd import hip
    refs, reads = edges.pool_pressure()
    mat = np.asarray(edges.blosum62(), dtype=np.int8)
    rd, ro = hip.pack(reads); fd, fo = hip.pack(refs)
    rows, cig = ctx.ssw_batch(rd, ro, fd, fo, mat, 11, 1, flag=1, score_size=2, want_score2=True, want_cigar=True)
    n_trunc = sum(bool(int(r['status']) & hip.ST_CIGAR_TRUNC) for r in rows)
    assert n_trunc == 0, '%d of %d CIGARs truncated' % (n_trunc, len(rows))
    _check_against_oracle(rows, cig, refs, reads, mat, 11, 1, 'pool')
