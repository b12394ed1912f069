"""tools/edit_align_model.py (the block recurrences of K4m / K4t per mode, and the traceback from stored vectors) against
tests/edlib_check.py (the plain dynamic programme), on seeded pairs of every mode.  CPU only."""
import os
import random
import sys

import pytest

import edlib_check

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
import edit_align_model as model  # noqa: E402


def _pair(rng, m, n, alpha, plant):
    q = bytes(rng.choice(alpha) for _ in range(m))
    t = bytes(rng.choice(alpha) for _ in range(n))
    if plant and m and n > m:
        p = rng.randint(0, n - m)
        core = bytearray(q)
        for _ in range(rng.randint(0, max(1, m // 8))):
            core[rng.randrange(len(core))] = rng.choice(alpha)
        t = t[:p] + bytes(core) + t[p + m:]
    return q, t


@pytest.mark.parametrize('mode', ['NW', 'SHW', 'HW'])
def test_model_equals_checker(mode):
    rng = random.Random({'NW': 1, 'SHW': 2, 'HW': 3}[mode])
    for it in range(120):
        m = rng.choice([0, 1, 2, 63, 64, 65, 127, 128, 129, rng.randint(1, 200)])
        q, t = _pair(rng, m, rng.randint(0, 260), b'ACGT' if it % 2 else b'ACGTN', it % 3 == 0)
        for task in ('distance', 'locations', 'path'):
            got = model.align(q, t, mode, task)
            assert got == edlib_check.align(q, t, mode, task), (q, t, task)
            edlib_check.check_invariants(got, q, t, mode)


@pytest.mark.parametrize('mode', ['NW', 'SHW', 'HW'])
def test_model_tandem_repeats_and_homopolymers(mode):
    rng = random.Random(7)
    for it in range(60):
        unit = bytes(rng.choice(b'ACGT') for _ in range(rng.randint(1, 4)))
        t = (unit * 80)[:rng.randint(1, 300)]
        q = (unit * 40)[:rng.randint(1, 130)] if it % 2 else bytes([unit[0]]) * rng.randint(1, 70)
        got = model.align(q, t, mode, 'path')
        assert got == edlib_check.align(q, t, mode, 'path'), (q, t)


def test_model_above_4096_rows():
    rng = random.Random(11)
    for m in (4097, 4200):
        q, t = _pair(rng, m, 40, b'ACGT', False)
        t = q[1000:1030] + t
        for mode in ('NW', 'SHW', 'HW'):
            assert model.align(q, t, mode, 'locations') == edlib_check.align(q, t, mode, 'locations')
    q, t = _pair(rng, 4150, 4170, b'ACGT', True)
    assert model.align(q, t, 'HW', 'path') == edlib_check.align(q, t, 'HW', 'path')


def test_model_additional_equalities():
    rng = random.Random(13)
    eq = [(ord('N'), ord('A')), (ord('N'), ord('C')), (ord('R'), ord('G')), (ord('R'), ord('A'))]
    for it in range(80):
        q, t = _pair(rng, rng.randint(1, 150), rng.randint(1, 200), b'ACGTNR', it % 2 == 0)
        for mode in ('NW', 'SHW', 'HW'):
            got = model.align(q, t, mode, 'path', eq=eq)
            assert got == edlib_check.align(q, t, mode, 'path', -1, eq), (q, t, mode)
            edlib_check.check_invariants(got, q, t, mode, eq)
    # not transitive: N = A and N = C do not make A = C
    assert edlib_check.align(b'A', b'C', 'NW', 'path', -1, eq)['cigar'] == '1X'
    assert model.align(b'A', b'C', 'NW', 'path', eq=eq)['cigar'] == '1X'


def test_issue_example_follows_from_the_dp():
    r = {'editDistance': 1, 'alphabetLength': 5, 'locations': [(1, 3), (1, 4)], 'cigar': '3=1I'}
    assert edlib_check.align('ACTG', 'CACTRT', 'HW', 'path') == r
    assert model.align(b'ACTG', b'CACTRT', 'HW', 'path') == r
