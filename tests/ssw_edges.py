"""Seeded Smith-Waterman cases at the edges where the DNA kernel classes are most likely to be wrong: the 16-bit score ceiling (the
reference's word pass saturates at 32767 and reports the first cell that reaches it), gap extensions above 16, general 5 x 5 matrices
(and edges 1..4), score_size 1 / 2 and flag 0 / 1.  The reference's answers live in tests/golden/ssw_edges_golden.json.gz (made by
tests/golden/make_ssw_edges_golden.py from oracle/_ref/libssw.so); tests/test_ssw_edges_host.py holds the CPU statement to them and
tests/test_gpu_ssw_edges.py the kernels.

A case is (reference, read, (match, mismatch, gap_open, gap_extend), keyword arguments of oracle_align / ref_align); the sequences are
strings over ACGTN, a general matrix travels as a flat n * n list under 'mat'."""
import json
import zlib

import numpy as np

GOLDEN_NAME = 'ssw_edges_golden.json.gz'
LETTERS = 'ACGTN'

# read lengths around the ceiling at match 10: 3199 * 10 < 32000 (K1w's bound) <= 3200 * 10; 3276 * 10 < 32767 <= 3277 * 10
CEILING_LENGTHS = (3199, 3200, 3276, 3277, 3300, 4000, 4096)
BIG_GAP_EXTENDS = (17, 33, 64, 127, 254)


def _s(codes):
    return ''.join(LETTERS[int(c)] for c in codes)


def _mutated(rng, core, rate, length):
    """core with substitutions / single-base insertions / deletions at `rate` (a third each), then cut or padded to `length`"""
    u = rng.random(len(core))
    out = []
    for c, x in zip(core, u):
        if x < rate / 3:
            continue
        if x < 2 * rate / 3:
            out.append(int(rng.integers(0, 4)))
            continue
        out.append(int(c))
        if x < rate:
            out.append(int(rng.integers(0, 4)))
    out = np.asarray(out[:length], dtype=np.int8)
    if len(out) < length:
        out = np.concatenate([out, rng.integers(0, 4, length - len(out), dtype=np.int8)])
    return out


def _copy_case(rng, L, rate, flank, read_flank=0, alpha=4):
    """a reference of random bases around a core; the read: the core (mutated at `rate`) with `read_flank` random bases on each side,
    L bases in all"""
    core_len = L - 2 * read_flank
    core = rng.integers(0, alpha, core_len, dtype=np.int8)
    ref = np.concatenate([rng.integers(0, alpha, flank, dtype=np.int8), core, rng.integers(0, alpha, flank // 2 + 1, dtype=np.int8)])
    body = core.copy() if rate == 0 else _mutated(rng, core, rate, core_len)
    q = np.concatenate([rng.integers(0, alpha, read_flank, dtype=np.int8), body, rng.integers(0, alpha, read_flank, dtype=np.int8)])
    return _s(ref), _s(q)


def ceiling(scheme, seed, rates=(0, 0.01, 0.02, 0.03)):
    """reads of CEILING_LENGTHS, perfect and mutated, against references with flanks: saturated, near-ceiling and just-below scores"""
    rng = np.random.default_rng(seed)
    cases = []
    for L in CEILING_LENGTHS:
        for rate in rates:
            rf = 0 if rate == 0 else int(rng.integers(0, 40))
            ref, q = _copy_case(rng, L, rate, int(rng.integers(30, 300)), rf)
            cases.append((ref, q, scheme, {}))
    return cases


def ceiling_long():
    """reads above 4096 bases that saturate at 10/4/8/2 (the anti-diagonal kernel's row strips)"""
    rng = np.random.default_rng(4097)
    return [(*_copy_case(rng, L, rate, 200, 10 if rate else 0), (10, 4, 8, 2), {}) for L, rate in ((4500, 0), (5000, 0.02), (8000, 0.01))]


def ceiling_match1():
    """match 1: reads of 32 767 bases and more -- exactly at the ceiling, and past it with mutations (two only: ~10^9 cells each)"""
    rng = np.random.default_rng(32767)
    return [(*_copy_case(rng, L, rate, 60), (1, 1, 1, 1), {}) for L, rate in ((32767, 0), (34000, 0.005))]


def big_gap_extend():
    """gap_extend 17..254 with gap_open equal and above it; reads that carry long indels so that the gap terms decide the path"""
    rng = np.random.default_rng(1717)
    cases = []
    for ge in BIG_GAP_EXTENDS:
        for go in sorted({ge, min(255, ge + 1), min(255, ge + 40)}):
            for L, scheme_m in ((60, 40), (200, 60), (700, 40), (1500, 20)):
                core = rng.integers(0, 4, L, dtype=np.int8)
                q = core.copy()
                for _ in range(int(rng.integers(1, 4))):        # long insertions and deletions in the read
                    p = int(rng.integers(5, len(q) - 5))
                    q = np.concatenate([q[:p], rng.integers(0, 4, int(rng.integers(1, 9)), dtype=np.int8), q[p:]]) if rng.random() < 0.5 \
                        else np.concatenate([q[:p], q[p + int(rng.integers(1, 6)):]])
                q = _mutated(rng, q, 0.03, len(q))
                ref = np.concatenate([rng.integers(0, 4, int(rng.integers(10, 200)), dtype=np.int8), core, rng.integers(0, 4, 50, dtype=np.int8)])
                cases.append((_s(ref), _s(q), (scheme_m, int(rng.integers(1, scheme_m)), go, ge), {}))
    return cases


def big_gap_extend_long():
    """gap_extend 64 and 127 on near-copies of ~9 000 bases: the row traceback leaves gap_extend > 60 to the anti-diagonal form, whose LDS
    does not hold 12 352 bases of read + reference"""
    rng = np.random.default_rng(6464)
    cases = []
    for L, (go, ge) in ((9000, (64, 64)), (9000, (100, 64)), (9500, (127, 127)), (9500, (200, 127))):
        core = rng.integers(0, 4, L, dtype=np.int8)
        q = core.copy()
        for _ in range(3):                                  # long indels the path crosses
            p = int(rng.integers(100, len(q) - 100))
            q = np.concatenate([q[:p], rng.integers(0, 4, int(rng.integers(3, 9)), dtype=np.int8), q[p:]]) if rng.random() < 0.5 \
                else np.concatenate([q[:p], q[p + int(rng.integers(3, 9)):]])
        q = _mutated(rng, q, 0.004, len(q))
        ref = np.concatenate([rng.integers(0, 4, 120, dtype=np.int8), core, rng.integers(0, 4, 80, dtype=np.int8)])
        cases.append((_s(ref), _s(q), (3, 2, go, ge), {}))
    return cases


def random_matrix(rng, n):
    """a well-formed n x n matrix (flat): positive diagonal over the bases, mismatches at most 0; for n = 5 the N row and column are 0
    (null code 4) or small non-zero values, possibly asymmetric"""
    m = np.zeros((n, n), dtype=np.int64)
    nb = min(n, 4)
    for i in range(nb):
        for j in range(nb):
            m[i, j] = int(rng.integers(1, 11)) if i == j else int(rng.integers(-9, 1))
    if n == 5 and rng.random() < 0.6:
        m[4, :] = rng.integers(-3, 2, 5)
        m[:, 4] = rng.integers(-3, 2, 5)
    return [int(v) for v in m.reshape(-1)]


def matrices():
    """general matrices: 5 x 5 (asymmetric, zero or non-zero N row / column) and edges 1..4, over reads of 30..600 bases"""
    rng = np.random.default_rng(55)
    cases = []
    for k in range(60):
        n = 5 if k < 40 else 1 + k % 4
        mat = random_matrix(rng, n)
        go = int(rng.integers(1, 12)); ge = int(rng.integers(1, go + 1))
        L = int(rng.choice([30, 120, 254, 400, 600]))
        alpha = min(n, 4)
        core = rng.integers(0, alpha, L, dtype=np.int8)
        ref = np.concatenate([rng.integers(0, alpha, int(rng.integers(0, 300)), dtype=np.int8), core, rng.integers(0, alpha, 40, dtype=np.int8)])
        q = _mutated(rng, core, 0.08, L) % alpha
        if n == 5:                                         # Ns in both sequences
            q = q.copy(); ref = ref.copy()
            q[rng.integers(0, L, 3)] = 4; ref[rng.integers(0, len(ref), 3)] = 4
        cases.append((_s(ref), _s(q), (0, 0, go, ge), {'mat': mat}))
    return cases


def score_size_flag():
    """score_size 1 / 2 and flag 0 / 1 below, across and above the 8-bit limit and at the 16-bit ceiling"""
    rng = np.random.default_rng(12)
    cases = []
    for score_size in (1, 2):
        for flag in (0, 1):
            for L, scheme in ((100, (2, 2, 3, 1)), (140, (2, 2, 3, 1)), (600, (2, 2, 3, 1)), (3300, (10, 4, 8, 2))):
                ref, q = _copy_case(rng, L, 0.02, 150, 5)
                cases.append((ref, q, scheme, {'score_size': score_size, 'flag': flag}))
    return cases


def all_cases():
    """every case set by its key in the golden file"""
    return {
        'ceiling 10/4/8/2': ceiling((10, 4, 8, 2), 10482),
        'ceiling 10/4/6/6': ceiling((10, 4, 6, 6), 10466, rates=(0, 0.02)),
        'ceiling long': ceiling_long(),
        'ceiling match 1': ceiling_match1(),
        'gap_extend above 16': big_gap_extend(),
        'gap_extend above 60, long': big_gap_extend_long(),
        'matrices': matrices(),
        'score_size and flag': score_size_flag(),
    }


def case_crc(case):
    ref, q, scheme, kw = case
    return zlib.crc32(json.dumps([ref, q, list(scheme), sorted(kw.items())]).encode()) & 0xffffffff


def call_args(case):
    """(ref, query, *scheme) and keyword arguments for oracle_align / ref_align"""
    ref, q, scheme, kw = case
    kw = dict(kw)
    if 'mat' in kw:
        kw['mat'] = np.asarray(kw['mat'], dtype=np.int8)      # flat n * n: a 2-D array would be read as n = 2
    return (ref, q) + tuple(scheme), kw
