"""Alignments over substitution matrices of 6..32 letters on the GPU (K1a, csrc/ssw_alpha.hip), bit-exact as whole result dicts with
CIGARs: against the reference's answers in tests/golden/ssw_alphabet_golden.json.gz, against the reference library itself
(oracle_lib.ref_align) and the CPU oracle on fresh seeded batches, through every entry point -- Context.ssw_batch, Context.plan,
the legacy ssw_init / ssw_align of libclh.so, ssw_wrap.align_pairs_matrix."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib
from oracle_lib import cigar_to_string, oracle_align
from test_ssw_alphabet_host import golden_args, load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    from ciri_long_amd import hip
    return hip.Context(0)


def as_dict(r, cig, qlen):
    """one GPU row in the shape oracle_align / ref_align return (None where the reference returns NULL)"""
    from ciri_long_amd import hip
    if int(r['status']) & (hip.ST_NULL | hip.ST_TRACE_ERR | hip.ST_CIGAR_TRUNC):
        return None
    cg = [int(x) for x in cig[r['cigar_off']:r['cigar_off'] + r['cigar_len']]] if r['cigar_len'] > 0 else []
    qb, qe = int(r['read_begin1']), int(r['read_end1'])
    return dict(score=int(r['score1']), score2=int(r['score2']), ref_begin=int(r['ref_begin1']), ref_end=int(r['ref_end1']),
                query_begin=qb, query_end=qe, ref_end2=int(r['ref_end2']), cigar=cg,
                cigar_string=cigar_to_string(cg, qb, qe, qlen) if cg else None)


def run_batch(ctx, refs, reads, mat, o, e, flag, score_size, masks, filters=0, filterd=0):
    from ciri_long_amd import hip
    rd, ro = hip.pack(reads)
    fd, fo = hip.pack(refs)
    rows, cig = ctx.ssw_batch(rd, ro, fd, fo, mat, o, e, flag=flag, score_size=score_size, want_score2=True, want_cigar=True,
                              mask_len=np.asarray(masks, dtype=np.int32), filters=filters, filterd=filterd)
    return [as_dict(rows[k], cig, len(reads[k])) for k in range(len(reads))]


def random_matrix(rng, n):
    m = rng.integers(-6, 1, size=(n, n))
    m = np.triu(m) + np.triu(m, 1).T
    np.fill_diagonal(m, rng.integers(1, 12, size=n))
    return m.astype(np.int8).reshape(-1)


def mutate(rng, s, n, p):
    out = []
    for c in s:
        u = rng.random()
        if u < p / 3:
            continue
        if u < 2 * p / 3:
            out.append(int(rng.integers(n))); continue
        out.append(int(c))
        if u < p:
            out.extend(int(x) for x in rng.integers(0, n, int(rng.integers(1, 6))))
    return np.array(out if out else [0], dtype=np.int8)


def fresh_pairs(rng, n, count, lmax=700, rmax=2500):
    refs, reads = [], []
    for _ in range(count):
        R = int(rng.integers(0, rmax))
        ref = rng.integers(0, n, R).astype(np.int8)
        L = int(rng.integers(1, lmax))
        if R > 10 and rng.random() < 0.7:
            a = int(rng.integers(0, max(1, R - L)))
            read = mutate(rng, ref[a:a + L], n, float(rng.choice([0.02, 0.1, 0.3])))
        else:
            read = rng.integers(0, n, L).astype(np.int8)
        refs.append(ref); reads.append(read)
    return refs, reads


def test_golden_bit_exact(ctx):
    """every golden case, batched by options (mixed lengths in one batch; maskLen per alignment)"""
    g = load_golden()
    groups = {}
    for k, c in enumerate(g['cases']):
        key = (c['mat'], c['gap_open'], c['gap_extend'], c['flag'], c['score_size'], c['filters'], c['filterd'])
        groups.setdefault(key, []).append(k)
    checked = 0
    for key, idx in groups.items():
        args = [golden_args(g, g['cases'][k]) for k in idx]
        kw = args[0][1]
        got = run_batch(ctx, [a[0][0] for a in args], [a[0][1] for a in args], kw['mat'], kw['gap_open'], kw['gap_extend'], kw['flag'],
                        kw['score_size'], [a[1]['maskl'] for a in args], kw['filters'], kw['filterd'])
        for k, gg in zip(idx, got):
            assert gg == g['cases'][k]['want'], (k, gg, g['cases'][k]['want'])
            checked += 1
    assert checked == len(g['cases'])


@pytest.mark.parametrize('n', [6, 20, 24, 32])
def test_fresh_batches_vs_reference_and_oracle(ctx, n):
    rng = np.random.default_rng(1000 + n)
    for score_size, flag, (o, e) in [(2, 1, (11, 1)), (2, 15, (5, 5)), (0, 1, (4, 2)), (1, 7, (3, 0))]:
        mat = random_matrix(rng, n)
        refs, reads = fresh_pairs(rng, n, 120)
        masks = [max(15, len(q) // 2) if rng.random() < 0.8 else int(rng.integers(1, 15)) for q in reads]
        got = run_batch(ctx, refs, reads, mat, o, e, flag, score_size, masks, filters=30, filterd=400)
        for k in range(len(reads)):
            kw = dict(gap_open=o, gap_extend=e, flag=flag, score_size=score_size, mat=mat, maskl=masks[k], filters=30, filterd=400)
            want = oracle_align(refs[k], reads[k], **kw)
            assert got[k] == want, (n, score_size, flag, k)
            if oracle_lib.have_ref():
                assert got[k] == oracle_lib.ref_align(refs[k], reads[k], **kw), (n, score_size, flag, k)


def test_plan_runs_twice(ctx):
    import torch
    from ciri_long_amd import hip
    rng = np.random.default_rng(77)
    mat = random_matrix(rng, 25)
    refs, reads = fresh_pairs(rng, 25, 300, lmax=1200)
    reads.append(rng.integers(0, 25, 9000).astype(np.int8))          # above the LDS form's 8192 rows: the global form
    refs.append(np.concatenate([rng.integers(0, 25, 500).astype(np.int8), reads[-1][:6000]]))
    rd, ro = hip.pack(reads); fd, fo = hip.pack(refs)
    d_r = torch.from_numpy(rd.view(np.uint8)).cuda(); d_f = torch.from_numpy(fd.view(np.uint8)).cuda()
    ts = torch.cuda.Stream()
    plan = ctx.plan(ro, fo, mat, 6, 2, flag=1, score_size=2, want_score2=True, want_cigar=True)
    assert all(-14 <= rv <= -10 for rv, _c, _a, _b in plan.segments())
    want = [oracle_align(refs[k], reads[k], gap_open=6, gap_extend=2, flag=1, score_size=2, mat=mat) for k in range(len(reads))]
    for _ in range(2):
        plan.run(d_r.data_ptr(), d_f.data_ptr(), ts.cuda_stream)
        rows, cig = plan.fetch()
        got = [as_dict(rows[k], cig, len(reads[k])) for k in range(len(reads))]
        assert got == want
    plan.close()


def test_codes_outside_the_matrix(ctx):
    from ciri_long_amd import hip
    mat = random_matrix(np.random.default_rng(3), 20)
    reads = [np.array([1, 2, 3], dtype=np.int8), np.array([1, 20, 3], dtype=np.int8)]
    refs = [np.array([1, 2, 3, 4], dtype=np.int8)] * 2
    with pytest.raises(hip.ClhError, match='alignment 1: a read or reference code outside'):
        run_batch(ctx, refs, reads, mat, 3, 1, 1, 2, [15, 15])
    rd, ro = hip.pack(reads); fd, fo = hip.pack([refs[0], np.array([1, -1, 3], dtype=np.int8)])
    import torch
    d_r = torch.from_numpy(rd.view(np.uint8)).cuda(); d_f = torch.from_numpy(fd.view(np.uint8)).cuda()
    torch.cuda.synchronize()
    plan = ctx.plan(ro, fo, mat, 3, 1)
    plan.run(d_r.data_ptr(), d_f.data_ptr())
    with pytest.raises(hip.ClhError, match='alignment 1: a read or reference code outside'):
        plan.fetch()
    plan.close()


def _legacy():
    from ciri_long_amd import hip
    L = C.CDLL(hip.SO_PATH)
    L.ssw_init.restype = C.c_void_p
    L.ssw_init.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int8]
    L.init_destroy.argtypes = [C.c_void_p]
    L.ssw_align.restype = C.POINTER(oracle_lib.CloAlign)
    L.ssw_align.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_uint8, C.c_uint8, C.c_uint8, C.c_uint16, C.c_int32, C.c_int32]
    L.align_destroy.argtypes = [C.POINTER(oracle_lib.CloAlign)]
    return L


def test_legacy_ssw_align_n24(ctx, capfd):
    from ciri_long_amd.ssw_wrap import BLOSUM62
    L = _legacy()
    mat = np.ascontiguousarray(BLOSUM62.reshape(-1))
    rng = np.random.default_rng(24)
    refs, reads = fresh_pairs(rng, 24, 40, lmax=400, rmax=1200)
    for k in range(len(reads)):
        q = np.ascontiguousarray(reads[k]); r = np.ascontiguousarray(refs[k])
        prof = L.ssw_init(q.ctypes.data, len(q), mat.ctypes.data, 24, 2)
        p = L.ssw_align(prof, r.ctypes.data, len(r), 11, 1, 1, 0, 0, max(15, len(q) // 2))
        assert p, k
        res = p.contents
        cg = [res.cigar[i] for i in range(res.cigarLen)]
        got = dict(score=res.score1, score2=res.score2, ref_begin=res.ref_begin1, ref_end=res.ref_end1, query_begin=res.read_begin1,
                   query_end=res.read_end1, ref_end2=res.ref_end2, cigar=cg,
                   cigar_string=cigar_to_string(cg, res.read_begin1, res.read_end1, len(q)) if cg else None)
        L.align_destroy(p); L.init_destroy(prof)
        want = oracle_align(r, q, gap_open=11, gap_extend=1, flag=1, score_size=2, mat=mat)
        assert got == want, k
    # score_size 0 and a score past the 8-bit pass: NULL with the reference's message
    q = np.ascontiguousarray(np.tile(np.arange(20, dtype=np.int8), 10)); r = np.ascontiguousarray(np.concatenate([q, q]))
    capfd.readouterr()
    prof = L.ssw_init(q.ctypes.data, len(q), mat.ctypes.data, 24, 0)
    p = L.ssw_align(prof, r.ctypes.data, len(r), 11, 1, 1, 0, 0, 100)
    L.init_destroy(prof)
    assert not p
    assert 'Please set 2 to the score_size parameter of the function ssw_init' in capfd.readouterr().err


def test_align_pairs_matrix_blosum62(ctx):
    from ciri_long_amd import ssw_wrap
    A = ssw_wrap.BLOSUM62_ALPHABET
    rng = np.random.default_rng(62)
    refs, reads = fresh_pairs(rng, 20, 80, lmax=500, rmax=1500)           # the 20 amino acids
    rs = [''.join(A[c] for c in r) for r in refs]
    qs = [''.join(A[c] for c in q).lower() for q in reads]
    got = ssw_wrap.align_pairs_matrix(rs, qs, ssw_wrap.BLOSUM62, A, 11, 1, report_secondary=True, report_cigar=True, context=ctx)
    mat = ssw_wrap.BLOSUM62.reshape(-1)
    for k in range(len(qs)):
        w = oracle_align(refs[k], reads[k], gap_open=11, gap_extend=1, flag=1, score_size=2, mat=mat)
        g = got[k]
        if w is None:
            assert g is None, k
            continue
        assert (g.score, g.ref_begin, g.ref_end, g.query_begin, g.query_end) == \
            (w['score'], w['ref_begin'], w['ref_end'], w['query_begin'], w['query_end']), k
        assert (g.score2, g.ref_end2) == ((w['score2'], w['ref_end2']) if w['score2'] != 0 else (None, None)), k
        assert g.cigar_string == w['cigar_string'], k


def protein_batch(count=20000, seed=20000):
    """protein-like pairs: a BLOSUM62 read of 100..500 residues, a mutated copy of it inside a reference of 1.0..1.5 x its length"""
    rng = np.random.default_rng(seed)
    refs, reads = [], []
    for _ in range(count):
        L = int(rng.integers(100, 501))
        read = rng.integers(0, 20, L).astype(np.int8)
        core = mutate(rng, read, 20, 0.25)
        R = int(L * rng.uniform(1.0, 1.5))
        ref = rng.integers(0, 20, max(R, len(core))).astype(np.int8)
        a = int(rng.integers(0, len(ref) - len(core) + 1))
        ref[a:a + len(core)] = core
        refs.append(ref); reads.append(read)
    return refs, reads


def test_protein_batch_20000(ctx):
    from ciri_long_amd import hip
    from ciri_long_amd.ssw_wrap import BLOSUM62
    refs, reads = protein_batch()
    mat = np.ascontiguousarray(BLOSUM62.reshape(-1))
    rd, ro = hip.pack(reads); fd, fo = hip.pack(refs)
    rows, cig = ctx.ssw_batch(rd, ro, fd, fo, mat, 11, 1, flag=1, score_size=2, want_score2=True, want_cigar=True)
    check = oracle_lib.ref_align if oracle_lib.have_ref() else oracle_align
    for k in range(len(reads)):
        assert as_dict(rows[k], cig, len(reads[k])) == check(refs[k], reads[k], gap_open=11, gap_extend=1, flag=1, score_size=2, mat=mat), k
