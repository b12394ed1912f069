"""edlib.align on the GPU (K4m / K4t, csrc/edit_align.hip): every case an exact dict equality against tests/edlib_check.py,
the plain dynamic programme."""
import random

import numpy as np
import pytest

import edlib_check

pytestmark = pytest.mark.gpu

MODES = ('NW', 'SHW', 'HW')
TASKS = ('distance', 'locations', 'path')
ALPHABETS = {'dna': b'ACGT', 'dnan': b'ACGTN', 'aa20': b'ACDEFGHIKLMNPQRSTVWY', 'bytes': bytes(range(256))}


@pytest.fixture(scope='module')
def ctx():
    from ciri_long_amd import hip
    c = hip.Context(0)
    yield c
    c.close()


def _mutate(rng, s, rate, alpha):
    out = bytearray()
    for ch in s:
        r = rng.random()
        if r < rate / 3:
            out.append(rng.choice(alpha))
        elif r < 2 * rate / 3:
            continue
        elif r < rate:
            out.append(ch); out.append(rng.choice(alpha))
        else:
            out.append(ch)
    return bytes(out)


def _pairs(seed, alpha, count=48):
    """queries of 1..300 letters (across 64-row block edges) in targets that hold a mutated copy, tandem repeats or homopolymers"""
    rng = random.Random(seed)
    qs, ts = [], []
    for i in range(count):
        m = rng.choice([1, 2, 20, 63, 64, 65, 128, 129, rng.randint(3, 300)])
        kind = i % 4
        if kind == 0:     # tandem repeat target: many end locations and ties
            unit = bytes(rng.choice(alpha) for _ in range(rng.randint(1, 6)))
            t = (unit * (400 // len(unit) + 1))[:rng.randint(1, 400)]
            q = _mutate(rng, (unit * (m // len(unit) + 1))[:m], rng.choice([0, 0.1, 0.4]), alpha)
        elif kind == 1:   # homopolymer runs
            t = b''.join(bytes([rng.choice(alpha)]) * rng.randint(1, 30) for _ in range(rng.randint(1, 20)))
            q = bytes([rng.choice(alpha)]) * m
        else:             # a copy at 0..40 % divergence inside random flanks
            q = bytes(rng.choice(alpha) for _ in range(m))
            core = _mutate(rng, q, rng.choice([0, 0.05, 0.1, 0.2, 0.4]), alpha)
            t = bytes(rng.choice(alpha) for _ in range(rng.randint(0, 200))) + core + bytes(rng.choice(alpha) for _ in range(rng.randint(0, 200)))
        qs.append(q or bytes([alpha[0]])); ts.append(t)
    return qs, ts


def _check(qs, ts, got, mode, task, k=-1, eq=None):
    for q, t, g in zip(qs, ts, got):
        want = edlib_check.align(q, t, mode, task, k, eq)
        assert g == want, (mode, task, q[:60], t[:60], g, want)
        edlib_check.check_invariants(g, q, t, mode, eq)


def test_issue_example(ctx):
    from ciri_long_amd import edlib
    r = edlib.align('ACTG', 'CACTRT', mode='HW', task='path')
    assert r == {'editDistance': 1, 'alphabetLength': 5, 'locations': [(1, 3), (1, 4)], 'cigar': '3=1I'}
    assert r == edlib_check.align('ACTG', 'CACTRT', 'HW', 'path')


@pytest.mark.parametrize('alpha', sorted(ALPHABETS))
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('task', TASKS)
def test_seeded_batches(ctx, alpha, mode, task):
    from ciri_long_amd import edlib
    qs, ts = _pairs(100 * sorted(ALPHABETS).index(alpha) + 10 * MODES.index(mode) + TASKS.index(task), ALPHABETS[alpha])
    _check(qs, ts, edlib.align_batch(qs, ts, mode, task, context=ctx), mode, task)


@pytest.mark.parametrize('mode', MODES)
def test_additional_equalities(ctx, mode):
    from ciri_long_amd import edlib
    eq = [('N', 'A'), ('N', 'C'), ('N', 'G'), ('N', 'T'), ('R', 'A'), ('R', 'G')]
    qs, ts = _pairs(77, b'ACGTNR', 40)
    _check(qs, ts, edlib.align_batch(qs, ts, mode, 'path', additionalEqualities=eq, context=ctx), mode, 'path', eq=eq)


def test_nw_distance_equals_k4(ctx):
    from ciri_long_amd import edlib, utils
    qs, ts = _pairs(5, b'ACGTN', 64)
    got = [r['editDistance'] for r in edlib.align_batch(qs, ts, 'NW', 'distance', context=ctx)]
    assert got == [int(d) for d in utils.distance_batch([q.decode() for q in qs], [t.decode() for t in ts])]


@pytest.mark.parametrize('mode', MODES)
def test_k_bound(ctx, mode):
    from ciri_long_amd import edlib
    qs, ts = _pairs(9, b'ACGT', 24)
    for task in TASKS:
        free = edlib.align_batch(qs, ts, mode, task, context=ctx)
        for q, t, f in zip(qs, ts, free):
            d = f['editDistance']
            assert edlib.align(q, t, mode, task, k=d) == f                                   # a best equal to k is kept
            if d > 0:
                r = edlib.align(q, t, mode, task, k=d - 1)                                   # a best of k + 1 is not
                assert r == {'editDistance': -1, 'alphabetLength': f['alphabetLength'], 'locations': [], 'cigar': None}
                assert r == edlib_check.align(q, t, mode, task, d - 1)


@pytest.mark.parametrize('mode', MODES)
def test_queries_above_4096(ctx, mode):
    from ciri_long_amd import edlib
    rng = random.Random(41)
    qs, ts = [], []
    for m in (4097, 4160, 5000):
        q = bytes(rng.choice(b'ACGT') for _ in range(m))
        ts.append(bytes(rng.choice(b'ACGT') for _ in range(rng.randint(0, 300))) + _mutate(rng, q, 0.08, b'ACGT') +
                  bytes(rng.choice(b'ACGT') for _ in range(rng.randint(0, 300))))
        qs.append(q)
    _check(qs, ts, edlib.align_batch(qs, ts, mode, 'path', context=ctx), mode, 'path')


def test_hw_in_one_megabase_target(ctx):
    from ciri_long_amd import edlib
    rng = np.random.Generator(np.random.PCG64(3))
    t = bytes(rng.choice(np.frombuffer(b'ACGT', dtype=np.uint8), 1 << 20).tobytes())
    qs, ts = [], []
    for L, pos in ((24, 1000), (120, 500000), (200, (1 << 20) - 201)):
        qs.append(_mutate(random.Random(L), t[pos:pos + L], 0.1, b'ACGT')); ts.append(t)
    _check(qs, ts, edlib.align_batch(qs, ts, 'HW', 'path', context=ctx), 'HW', 'path')


@pytest.mark.parametrize('mode', MODES)
def test_empty_and_length_one(ctx, mode):
    from ciri_long_amd import edlib
    cases = [(b'', b''), (b'', b'A'), (b'', b'ACGT'), (b'A', b''), (b'ACGT', b''), (b'A', b'A'), (b'A', b'C'), (b'A', b'CAC'),
             (b'ACG', b'A'), (b'A', b'CCCC'), (b'\x00', b'\xff\x00')]
    for task in TASKS:
        got = edlib.align_batch([q for q, _ in cases], [t for _, t in cases], mode, task, context=ctx)
        _check([q for q, _ in cases], [t for _, t in cases], got, mode, task)
    # HW with an empty query: every column (and -1) is an end, start = end + 1
    assert edlib.align('', 'ACG', 'HW', 'locations')['locations'] == [(0, -1), (1, 0), (2, 1), (3, 2)]


def test_path_over_workspace_limit_raises(ctx):
    from ciri_long_amd import edlib, hip
    q = 'ACGT' * 300
    with pytest.raises(hip.ClhError):
        edlib.align_batch([q], [q], 'NW', 'path', context=ctx, workspace_bytes=1 << 16)
    # the same pair below the limit, and a batch that only fits in several chunks
    assert edlib.align_batch([q], [q], 'NW', 'path', context=ctx, workspace_bytes=1 << 20)[0]['cigar'] == '1200='
    qs, ts = _pairs(13, b'ACGT', 30)
    _check(qs, ts, edlib.align_batch(qs, ts, 'HW', 'path', context=ctx, workspace_bytes=1 << 18), 'HW', 'path')


def test_plan_runs_twice_like_the_batch(ctx):
    from ciri_long_amd import edlib
    qs, ts = _pairs(21, b'ACGTN', 40)
    want = edlib.align_batch(qs, ts, 'HW', 'path', context=ctx)
    plan = ctx.edit_align_plan(qs, ts, 'HW', 'path')
    try:
        for _ in range(2):
            plan.run()
            assert edlib.results_from_rows(*plan.fetch(), task='path') == want
            assert plan.timing() > 0
    finally:
        plan.close()
