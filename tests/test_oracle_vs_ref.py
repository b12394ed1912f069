"""Randomized check of the restatement against the reference's own ssw.c on seeded cases.  The reference's answers are stored in
tests/golden/oracle_vs_ref_golden.json.gz (made by tests/golden/make_oracle_vs_ref_golden.py from oracle/_ref/libssw.so, the
reference's ssw.c compiled by oracle/Makefile), so the check runs everywhere; where that library is built, every case also goes through
it and must give the stored answer."""
import gzip
import json
import os
import zlib

import numpy as np
import pytest

from oracle_lib import have_ref, oracle_align, ref_align

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'oracle_vs_ref_golden.json.gz')
SCHEMES = [(1, 1, 1, 1), (10, 4, 8, 2), (2, 2, 3, 1), (3, 5, 7, 7), (2, 3, 0, 0)]
SCORE_SIZES = [0, 1, 2]
FLAGS = [0, 1, 2, 8]
FILTER_FLAGS = [2, 4, 6, 8, 10, 12, 14, 3, 5]


def _rnd(rng, n):
    return ''.join('ACGT'[i] for i in rng.integers(0, 4, n))


def _mutate(s, rng, p=0.12):
    out = []
    for c in s:
        u = rng.random()
        if u < p / 3:
            continue
        if u < 2 * p / 3:
            out.append('ACGT'[rng.integers(4)])
            continue
        out.append(c)
        if u < p:
            out.append('ACGT'[rng.integers(4)])
    return ''.join(out)


# The cases: lists of (reference, query, (match, mismatch, gap_open, gap_extend), keyword arguments of the call)
def random_pairs(scheme):
    rng = np.random.default_rng(hash(scheme) & 0xffff)
    cases = []
    for _ in range(250):
        L = int(rng.choice([21, 33, 64, 130, 255, 300, 520]))
        R = int(rng.choice([40, 300, 900]))
        ref = _rnd(rng, R)
        st = int(rng.integers(0, max(1, R - L)))
        q = _mutate(ref[st:st + L], rng)
        if rng.random() < 0.25:
            q = q + q[: len(q) // 2]
        if rng.random() < 0.15:
            ref = ref[: R // 3] + 'N' * 9 + ref[R // 3:]
        if not q:
            continue
        cases.append((ref, q, scheme, {}))
    return cases


def long_vertical_gaps():
    rng = np.random.default_rng(7)
    cases = []
    for _ in range(150):
        L = int(rng.integers(300, 500))
        ref = _rnd(rng, 700)
        core = ref[100:100 + L]
        # drop long chunks from the reference side so the read carries long insertions
        q = core
        for _k in range(int(rng.integers(1, 6))):
            p = int(rng.integers(10, len(q) - 10))
            q = q[:p] + _rnd(rng, int(rng.integers(2, 12))) + q[p:]
        cases += [(ref, q, (1, 1, 1, 1), {}), (ref, q, (10, 4, 8, 2), {})]
    return cases


def score_size_variants(score_size):
    rng = np.random.default_rng(11 + score_size)
    cases = []
    for _ in range(80):
        L = int(rng.choice([30, 200, 400]))
        ref = _rnd(rng, 600)
        q = _mutate(ref[50:50 + L], rng)
        cases.append((ref, q, (1, 1, 1, 1), {'score_size': score_size}))
    return cases


def flag_variants(flag):
    rng = np.random.default_rng(5)
    cases = []
    for _ in range(40):
        ref = _rnd(rng, 400)
        q = _mutate(ref[50:250], rng)
        cases.append((ref, q, (2, 2, 3, 1), {'flag': flag}))
    return cases


def flag_bits_with_filters(flag):
    rng = np.random.default_rng(600 + flag)
    cases = []
    for _ in range(60):
        ref = _rnd(rng, int(rng.integers(200, 700)))
        q = _mutate(ref[50:50 + int(rng.choice([30, 60, 120, 250]))], rng)
        cases.append((ref, q, (1, 1, 1, 1), {'flag': flag, 'filters': 55, 'filterd': 100}))
    return cases


def all_cases():
    """every case set by its key in the golden file"""
    out = {'random_pairs %s' % (s,): random_pairs(s) for s in SCHEMES}
    out['long_vertical_gaps'] = long_vertical_gaps()
    out.update({'score_size %d' % s: score_size_variants(s) for s in SCORE_SIZES})
    out.update({'flag %d' % f: flag_variants(f) for f in FLAGS})
    out.update({'flag_filters %d' % f: flag_bits_with_filters(f) for f in FILTER_FLAGS})
    return out


def case_crc(case):
    ref, q, scheme, kw = case
    return zlib.crc32(json.dumps([ref, q, list(scheme), sorted(kw.items())]).encode()) & 0xffffffff


_golden = None


def check(key, cases):
    """every case: the restatement gives the reference's stored answer (and so does the reference's library, where it is built).
    Returns the answers."""
    global _golden
    if _golden is None:
        with gzip.open(GOLDEN, 'rt') as f:
            _golden = json.load(f)['cases']
    want = _golden[key]
    assert len(want) == len(cases), key
    for k, (case, w) in enumerate(zip(cases, want)):
        assert case_crc(case) == w['crc'], 'case %d of %s is not the one the golden file was made from' % (k, key)
        ref, q, scheme, kw = case
        assert oracle_align(ref, q, *scheme, **kw) == w['want'], (key, k)
        if have_ref():
            assert ref_align(ref, q, *scheme, **kw) == w['want'], ('the reference library disagrees with the golden file', key, k)
    return [w['want'] for w in want]


@pytest.mark.parametrize('scheme', SCHEMES)
def test_random_pairs(scheme):
    check('random_pairs %s' % (scheme,), random_pairs(scheme))


def test_long_vertical_gaps_across_stripe_boundaries():
    """gap_open <= gap_extend: the 16-bit pass truncates vertical gaps at stripe starts (ssw.c:468-478)."""
    check('long_vertical_gaps', long_vertical_gaps())


@pytest.mark.parametrize('score_size', SCORE_SIZES)
def test_score_size_variants(score_size):
    check('score_size %d' % score_size, score_size_variants(score_size))


@pytest.mark.parametrize('flag', FLAGS)
def test_flag_variants(flag):
    check('flag %d' % flag, flag_variants(flag))


@pytest.mark.parametrize('flag', FILTER_FLAGS)
def test_flag_bits_with_filters(flag):
    """flag bits 1/2 with thresholds that split the inputs (ssw.c:834, 850): the scalar statement equals the reference's
    own library on every field and CIGAR (the GPU test of the same name holds the kernels to the statement)."""
    got = check('flag_filters %d' % flag, flag_bits_with_filters(flag))
    n_with = sum(bool(a['cigar']) for a in got)
    n_without = sum(not a['cigar'] for a in got)
    assert not (flag & 6) or (n_with > 0 and n_without > 0)
