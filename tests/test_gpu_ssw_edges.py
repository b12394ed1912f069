"""The DNA Smith-Waterman kernel classes at their routing edges and at the 16-bit score ceiling, bit-exact against the CPU statement of the
reference's passes (oracle/ssw_oracle.c) and, for the cases of tests/ssw_edges.py, against the reference's own answers stored in
tests/golden/ssw_edges_golden.json.gz.

Every routing test builds a batch on both sides of one threshold of clh_ssw_plan (csrc/clh_api.hip: scan_class_ok, scanw_class_ok,
scanw_sliced_ok, lanes_class_for) and first asserts, from plan.segments(), which class takes each side -- so that a later routing change
cannot silently stop testing the edge -- then compares every field, the status bits and the CIGAR."""
import ctypes as C
import gzip
import json
import os

import numpy as np
import pytest

import oracle_lib
import ssw_edges

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
# class codes of csrc/clh_device.h; the anti-diagonal K1 classes are the positive ones (rows per lane, 1000 = row strips)
K1S, K1S_SLICED, K1W, K1W_SLICED, K1W_TR = 0, -1, -3, -4, -9
LANES = (-5, -6, -7, -8)
STRIPS = 1000
SWITCHES = (None, 'CLH_NO_LANES', 'CLH_NO_SCANW')


def _golden():
    with gzip.open(os.path.join(HERE, 'golden', ssw_edges.GOLDEN_NAME), 'rt') as f:
        return json.load(f)['cases']


def _codes(s):
    return s if isinstance(s, np.ndarray) else oracle_lib.encode(s)


def _mat(scheme, mat):
    from ciri_long_amd import hip
    return np.asarray(mat, dtype=np.int8) if mat is not None else hip.score_matrix(scheme[0], scheme[1])


def classes(refs, qs, scheme, mat=None, score_size=2, flag=1, want_score2=True):
    """{class: alignments} of the plan clh_ssw_plan makes for the batch (the classes of csrc/clh_device.h)"""
    from ciri_long_amd import hip
    ctx = hip.default_context()
    _rd, ro = hip.pack([_codes(q) for q in qs]); _fd, fo = hip.pack([_codes(r) for r in refs])
    plan = ctx.plan(ro, fo, _mat(scheme, mat), scheme[2], scheme[3], flag=flag, score_size=score_size, want_score2=want_score2, want_cigar=True)
    seg = plan.segments()
    plan.close()
    out = {}
    for rv, n, _a, _b in seg:
        out[rv] = out.get(rv, 0) + n
    return out


def k1(cls):
    """alignments in the anti-diagonal K1 classes"""
    return sum(n for rv, n in cls.items() if rv > 0)


def run_and_check(refs, qs, scheme, mat=None, score_size=2, flag=1, want_score2=True, golden=None, tag=''):
    """the batch through clh_ssw_batch; every row equal to the oracle's answer (and to the golden answer where one is given): scores, ends,
    begins, second best (where asked for), the status bits and the CIGAR"""
    from ciri_long_amd import hip
    ctx = hip.default_context()
    rq = [_codes(q) for q in qs]; rf = [_codes(r) for r in refs]
    rd, ro = hip.pack(rq); fd, fo = hip.pack(rf)
    m = _mat(scheme, mat)
    rows, cig = ctx.ssw_batch(rd, ro, fd, fo, m, scheme[2], scheme[3], flag=flag, score_size=score_size, want_score2=want_score2, want_cigar=True)
    bias = -min(0, int(m.min()))
    for k in range(len(qs)):
        w = golden[k] if golden is not None else oracle_lib.oracle_align(rf[k], rq[k], *scheme, flag=flag, score_size=score_size,
                                                                         mat=None if mat is None else m)
        r = rows[k]
        got = dict(score=int(r['score1']), ref_begin=int(r['ref_begin1']), ref_end=int(r['ref_end1']), query_begin=int(r['read_begin1']),
                   query_end=int(r['read_end1']), cigar=[int(c) for c in cig[r['cigar_off']:r['cigar_off'] + r['cigar_len']]])
        exp = {f: w[f] for f in got}
        if want_score2:
            got.update(score2=int(r['score2']), ref_end2=int(r['ref_end2'])); exp.update(score2=w['score2'], ref_end2=w['ref_end2'])
        where = (tag, k, len(rq[k]), len(rf[k]), scheme)
        assert got == exp, where
        word = score_size == 1 or w['score'] + bias >= 255
        assert int(r['status']) == (hip.ST_WORD if word else 0) | (0 if flag & 7 else hip.ST_NO_CIGAR), where
    return rows


# ---------------------------------------------------------------------------------------------------------------------------------------
# the golden sets: the 16-bit ceiling, gap extensions above 16, general matrices, score_size / flag -- through the default routing and
# with K1l / K1w switched off, and with every CIGAR from the anti-diagonal traceback (CLH_NO_TB_ROWS)
# ---------------------------------------------------------------------------------------------------------------------------------------
def _golden_groups(key):
    """the cases of a golden set, grouped into batches of one option set"""
    cases = ssw_edges.all_cases()[key]
    want = _golden()[key]
    groups = {}
    for c, w in zip(cases, want):
        assert ssw_edges.case_crc(c) == w['crc'], key
        ref, q, scheme, kw = c
        gk = (tuple(scheme), tuple(kw.get('mat', ())), kw.get('score_size', 2), kw.get('flag', 1))
        groups.setdefault(gk, []).append((ref, q, w['want']))
    return groups


def check_golden_set(key):
    n_k1 = n_sat = 0
    for (scheme, mat, score_size, flag), items in _golden_groups(key).items():
        refs = [i[0] for i in items]; qs = [i[1] for i in items]; want = [i[2] for i in items]
        cls = classes(refs, qs, scheme, mat or None, score_size, flag)
        n_k1 += k1(cls)
        n_sat += sum(w['score'] == 32767 for w in want)
        run_and_check(refs, qs, scheme, mat or None, score_size, flag, golden=want, tag='%s %s' % (key, cls))
    return n_k1, n_sat


@pytest.mark.parametrize('switch', SWITCHES)
@pytest.mark.parametrize('key', list(ssw_edges.all_cases()))
def test_golden_edges(key, switch, monkeypatch):
    for s in SWITCHES[1:]:
        monkeypatch.delenv(s, raising=False)
    if switch:
        monkeypatch.setenv(switch, '1')
    n_k1, n_sat = check_golden_set(key)
    if key.startswith('ceiling'):
        assert n_sat > 0 and n_k1 >= n_sat, (key, n_k1, n_sat)           # the saturated alignments ran in the anti-diagonal classes


def test_golden_edges_anti_diagonal_traceback(monkeypatch):
    """every golden set again with every CIGAR from the anti-diagonal traceback kernel (CLH_NO_TB_ROWS=1)"""
    monkeypatch.setenv('CLH_NO_TB_ROWS', '1')
    for k in ssw_edges.all_cases():
        check_golden_set(k)


# ---------------------------------------------------------------------------------------------------------------------------------------
# routing thresholds: each side in the intended class, every answer equal to the oracle
# ---------------------------------------------------------------------------------------------------------------------------------------
def _pair(rng, L, R, related=True):
    """a reference of R bases and a read of L bases that holds a noisy copy of (part of) it"""
    from ciri_long_amd import synth
    ref = rng.integers(0, 4, R, dtype=np.int8)
    q = rng.integers(0, 4, L, dtype=np.int8)
    if related:
        n = min(L, R)
        a = int(rng.integers(0, R - n + 1))
        core = synth.mutate(ref[a:a + n], rng, sub=0.03, ins=0.02, dele=0.02)[:L]
        b = int(rng.integers(0, L - len(core) + 1))
        q[b:b + len(core)] = core
    return ref, q


def _sides(seed, shapes, copies=3):
    rng = np.random.default_rng(seed)
    out = []
    for L, R in shapes:
        refs, qs = zip(*[_pair(rng, L, R, related=(i % 3 != 2)) for i in range(copies)])
        out.append((list(refs), list(qs)))
    return out


def edge(seed, scheme, sides, want, want_score2=True, copies=3, **kw):
    """sides: [(L, R)], want: the class (or a predicate over the classes) of each side"""
    batches = _sides(seed, sides, copies)
    refs, qs = [], []
    for (rf, rq), (L, R), exp in zip(batches, sides, want):
        cls = classes(rf, rq, scheme, want_score2=want_score2, **kw)
        ok = exp(cls) if callable(exp) else cls == {exp: len(rf)}
        assert ok, ('side', L, R, scheme, cls, exp)
        refs += rf; qs += rq
    run_and_check(refs, qs, scheme, want_score2=want_score2, tag=str(sides), **kw)


def only_k1(cls):
    return bool(cls) and all(rv > 0 for rv in cls)


def test_read_length_254_255():
    """K1s takes reads of at most 254 bases (mismatch 0: the score bound is not what decides)"""
    edge(1, (1, 0, 2, 1), [(254, 400), (255, 400)], [K1S, K1W])


def test_score_bound_254_255():
    """K1s takes max_match * L + bias < 255: 253 + 1 = 254 stays, 254 + 1 = 255 goes to K1w"""
    edge(2, (1, 1, 2, 1), [(253, 400), (254, 400)], [K1S, K1W])


def test_cells_2048_2049():
    """K1l takes references of <= 64 columns up to 2048 cells when few alignments want it; 2049 cells go to the transposed K1w"""
    edge(3, (10, 4, 8, 2), [(32, 64), (683, 3), (64, 32), (33, 64)], [-8, K1W_TR, -6, K1W_TR], want_score2=False)


def test_cells_262144_262145_with_many_short_references():
    """with >= 32 768 K1l candidates in the batch, K1l takes up to 262 144 cells (64 x 4096); 262 145 (37 x 7085) go to the transposed
    K1w.  The filler alignments are checked on a sample."""
    from ciri_long_amd import hip
    rng = np.random.default_rng(262144)
    scheme = (10, 4, 8, 2)
    fill = [_pair(rng, 16, 16) for _ in range(32768)]
    edges = [_pair(rng, 4096, 64), _pair(rng, 4096, 64), _pair(rng, 7085, 37), _pair(rng, 7085, 37)]
    refs = [e[0] for e in edges] + [f[0] for f in fill]; qs = [e[1] for e in edges] + [f[1] for f in fill]
    cls = classes(refs, qs, scheme, want_score2=False)
    assert cls == {-8: 2, K1W_TR: 2, -5: len(fill)}, cls
    ctx = hip.default_context()
    rd, ro = hip.pack(qs); fd, fo = hip.pack(refs)
    rows, cig = ctx.ssw_batch(rd, ro, fd, fo, hip.score_matrix(10, 4), 8, 2, want_score2=False, want_cigar=True)
    for k in list(range(4)) + [int(x) for x in rng.integers(4, len(refs), 300)]:
        w = oracle_lib.oracle_align(refs[k], qs[k], *scheme)
        r = rows[k]
        got = (int(r['score1']), int(r['ref_begin1']), int(r['ref_end1']), int(r['read_begin1']), int(r['read_end1']),
               [int(c) for c in cig[r['cigar_off']:r['cigar_off'] + r['cigar_len']]], int(r['status']))
        assert got == (w['score'], w['ref_begin'], w['ref_end'], w['query_begin'], w['query_end'], w['cigar'],
                       hip.ST_WORD if w['score'] + 4 >= 255 else 0), (k, len(qs[k]), len(refs[k]))


def test_reference_64_65():
    edge(5, (2, 2, 3, 1), [(30, 64), (30, 65)], [-8, K1S], want_score2=False)


def test_transposed_read_lengths_4096_4097_32767_32768():
    """the transposed K1w takes reads up to 32 767 bases against references of <= 64 columns; 32 768 go to the row strips of K1"""
    edge(6, (10, 4, 8, 2), [(4096, 10), (4097, 10), (32767, 10), (32768, 10)], [K1W_TR, K1W_TR, K1W_TR, STRIPS], want_score2=False, copies=2)


def test_read_length_4096_4097():
    """K1w takes reads up to 4096 bases; 4097 go to K1's row strips"""
    edge(7, (1, 1, 1, 1), [(4096, 4500), (4097, 4500)], [K1W, STRIPS], copies=2)


def test_window_32767_32768():
    """K1s / K1w take windows below 32 768 columns; from there the sliced classes (call-path options) or K1 (second best wanted)"""
    edge(8, (1, 1, 1, 1), [(100, 32767), (100, 32768)], [K1S, K1S_SLICED], want_score2=False, copies=2)
    edge(9, (2, 2, 3, 1), [(300, 32767), (300, 32768)], [K1W, K1W_SLICED], want_score2=False, copies=2)
    edge(10, (2, 2, 3, 1), [(300, 32767), (300, 32768)], [K1W, only_k1], want_score2=True, copies=2)


def test_gap_open_255():
    """the largest gap_open (an 8-bit argument of ssw_align) in K1s, K1w, K1l and the transposed K1w"""
    edge(11, (10, 4, 255, 1), [(20, 300), (1000, 1400), (25, 40), (3000, 12)], [K1S, K1W, -7, K1W_TR], want_score2=False)
    edge(12, (10, 4, 255, 16), [(20, 300), (1000, 1400)], [K1S, K1W])


def test_gap_extend_16_17():
    """K1s, K1w and the sliced K1w need gap_extend <= 16; above it the alignments go to K1 (the transposed K1w and K1l keep them)"""
    edge(13, (10, 4, 20, 16), [(20, 300), (1000, 1400)], [K1S, K1W])
    edge(14, (10, 4, 20, 17), [(20, 300), (1000, 1400)], [only_k1, only_k1])
    edge(15, (2, 2, 20, 16), [(300, 40000)], [K1W_SLICED], want_score2=False, copies=2)
    # above 16: K1's window slices (5 of 8192 owned columns per 40 000-column window, one K1 class) and the combining step (-2)
    edge(16, (2, 2, 20, 17), [(300, 40000)], [lambda c: c.get(-2) == 2 and len(c) == 2 and all(0 < rv < STRIPS for rv in c if rv != -2) and
                                              sum(c.values()) == 2 + 2 * 5], want_score2=False, copies=2)


@pytest.mark.parametrize('switch', SWITCHES)
@pytest.mark.parametrize('ge', ssw_edges.BIG_GAP_EXTENDS)
def test_short_references_gap_extend_above_16(ge, switch, monkeypatch):
    """gap_extend 17..254 against references of <= 64 columns: K1l, the transposed K1w, and what takes them with those switched off"""
    for s in SWITCHES[1:]:
        monkeypatch.delenv(s, raising=False)
    if switch:
        monkeypatch.setenv(switch, '1')
    for go in sorted({ge, min(255, ge + 30)}):
        scheme = (40, 20, go, ge)
        batches = _sides(ge * 7 + go, [(20, 60), (3000, 50), (9000, 30)], copies=4)
        refs = sum((b[0] for b in batches), []); qs = sum((b[1] for b in batches), [])
        # long insertions in the reads: gaps worth opening
        rng = np.random.default_rng(ge + go)
        for k in range(len(qs)):
            p = int(rng.integers(1, len(qs[k]) - 1))
            qs[k] = np.concatenate([qs[k][:p], rng.integers(0, 4, 6, dtype=np.int8), qs[k][p:]])
        cls = classes(refs, qs, scheme, want_score2=False)
        # K1l takes the 26 x 60 reads, the transposed K1w the long ones -- not with gap_open == gap_extend (the 16-bit pass's own
        # recurrence), not with K1l switched off (the transposed class is its overflow), the transposed class not with K1w off; K1 the rest
        lanes_on = go > ge and switch != 'CLH_NO_LANES'
        n_l = 4 if lanes_on else 0
        n_tr = 8 if lanes_on and switch != 'CLH_NO_SCANW' else 0
        assert cls.get(-8, 0) == n_l and cls.get(K1W_TR, 0) == n_tr and k1(cls) == 12 - n_l - n_tr, (switch, go, ge, cls)
        run_and_check(refs, qs, scheme, want_score2=False, tag='ge %d go %d %s' % (ge, go, cls))


def test_legacy_six_symbols_saturated():
    """saturated alignments (a perfect 3 300-base copy at 10/4/8/2, a perfect 32 767-base copy at 1/1/1/1) through ssw_init / ssw_align
    of libclh.so, bound as the reference's Python wrapper binds them (ssw_wrap.py:54-72), against the reference's stored answers"""
    from ciri_long_amd import hip

    class CAlignRes(C.Structure):
        _fields_ = [('score', C.c_uint16), ('score2', C.c_uint16), ('ref_begin', C.c_int32), ('ref_end', C.c_int32),
                    ('query_begin', C.c_int32), ('query_end', C.c_int32), ('ref_end2', C.c_int32),
                    ('cigar', C.POINTER(C.c_uint32)), ('cigarLen', C.c_int32)]
    lib = C.CDLL(hip.SO_PATH)
    lib.ssw_init.restype = C.c_void_p
    lib.ssw_init.argtypes = [C.POINTER(C.c_int8), C.c_int32, C.POINTER(C.c_int8), C.c_int32, C.c_int8]
    lib.init_destroy.restype = None
    lib.init_destroy.argtypes = [C.c_void_p]
    lib.ssw_align.restype = C.POINTER(CAlignRes)
    lib.ssw_align.argtypes = [C.c_void_p, C.POINTER(C.c_int8), C.c_int32, C.c_uint8, C.c_uint8, C.c_uint8, C.c_uint16, C.c_int32, C.c_int32]
    lib.align_destroy.restype = None
    lib.align_destroy.argtypes = [C.POINTER(CAlignRes)]
    picked = [(c, w['want']) for c, w in zip(ssw_edges.all_cases()['ceiling 10/4/8/2'], _golden()['ceiling 10/4/8/2'])
              if len(c[1]) == 3300 and w['want']['score'] == 32767][:1]
    picked += [(c, w['want']) for c, w in zip(ssw_edges.all_cases()['ceiling match 1'], _golden()['ceiling match 1'])][:1]   # 32 767 bases, 1/1/1/1
    for (ref, q, scheme, _kw), want in picked:
        assert want['score'] == 32767 and want['cigar']
        qc = hip.encode(q); rc = hip.encode(ref); mat = hip.score_matrix(scheme[0], scheme[1])
        qa = (C.c_int8 * len(qc))(*qc.tolist()); ra = (C.c_int8 * len(rc))(*rc.tolist()); ma = (C.c_int8 * 25)(*mat.tolist())
        prof = lib.ssw_init(qa, len(qc), ma, 5, 2)
        res = lib.ssw_align(prof, ra, len(rc), scheme[2], scheme[3], 1, 0, 0, max(15, len(qc) // 2))
        assert res, len(q)
        a = res.contents
        got = dict(score=a.score, score2=a.score2, ref_begin=a.ref_begin, ref_end=a.ref_end, query_begin=a.query_begin, query_end=a.query_end,
                   ref_end2=a.ref_end2, cigar=[a.cigar[i] for i in range(a.cigarLen)])
        lib.align_destroy(res)
        lib.init_destroy(prof)
        assert got == {k: want[k] for k in got}, len(q)


def test_long_read_cigar_just_below_the_ceiling():
    """the row traceback takes a 32 766-base copy at match 1 (score 32 766 + bias 1 fits its 16-bit frame)"""
    rng = np.random.default_rng(32766)
    ref, q = ssw_edges._copy_case(rng, 32766, 0, 60)
    rows = run_and_check([ref], [q], (1, 1, 1, 1), tag='32766')
    assert int(rows[0]['cigar_len']) == 1 and int(rows[0]['score1']) == 32766
