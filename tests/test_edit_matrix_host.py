"""csrc/edit_matrix.hip without a GPU: the index arithmetic of its two kernels as tools/edit_matrix_model.py states it, against
np.triu_indices and utils.compress_seq, and the name of the A/B switch of the collapse route."""
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import edit_matrix_model as model  # noqa: E402


def test_pair_inversion_equals_triu_indices_for_every_small_n():
    for n in range(0, 131):
        ii, jj = np.triu_indices(n, 1)
        assert len(ii) == n * (n - 1) // 2
        got = [model.pair_of(q, n) for q in range(len(ii))]
        assert got == list(zip(ii.tolist(), jj.tolist())), n


@pytest.mark.parametrize('n', [2000, 46341, 65536])
def test_pair_inversion_at_the_row_borders_of_large_n(n):
    """first and last pair of every row: where a square root that is off by one ulp lands in the neighbouring row.  46 341 is the
    first n whose pair count passes 2^30, 65 536 the largest the API accepts (2^31 - 1 pairs)."""
    total = n * (n - 1) // 2
    assert total <= 2 ** 31 - 1
    for i in range(n - 1):
        first = model.row_start(i, n)
        last = first + (n - 1 - i) - 1
        assert model.pair_of(first, n) == (i, i + 1), (n, i)
        assert model.pair_of(last, n) == (i, n - 1), (n, i)
    assert model.row_start(n - 2, n) == total - 1
    if n == 2000:                                       # small enough to hold the whole triangle against numpy
        ii, jj = np.triu_indices(n, 1)
        rows = np.arange(n - 1)
        starts = np.array([model.row_start(int(i), n) for i in rows])
        assert (ii[starts] == rows).all() and (jj[starts] == rows + 1).all()


def test_keep_mask_and_wave_walk_equal_compress_seq():
    from ciri_long_amd import utils
    rng = random.Random(5)
    cases = ['', 'A', 'AA', 'A' * 300, 'ACGT' * 40, 'A' * 63 + 'C', 'A' * 64 + 'C', 'C' + 'A' * 64, 'AC' * 32 + 'CA' * 32]
    for _ in range(200):
        n = rng.randint(0, 400)
        cases.append(''.join(rng.choice('ACGT') * rng.choice((1, 1, 1, 2, 3, 70)) for _ in range(n))[:n])
    for s in cases:
        want = utils.compress_seq(s)
        assert ''.join(c for c, k in zip(s, model.keep_mask(s)) if k) == want
        assert ''.join(model.compress_waves(s)) == want


def test_lane_group_rule():
    assert [model.lane_group(m) for m in (1, 64, 65, 128, 129, 2048, 2049, 4096, 4097, 100000)] == [1, 1, 2, 2, 4, 32, 64, 64, 64, 64]


def test_the_switch_is_read_in_python_and_listed():
    text = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    sec = text[text.index('### Experiment / test hooks'):]
    assert '`CLH_NO_EDIT_MATRIX`' in sec[:sec.index('\n## 9.')]
    assert "environ.get('CLH_NO_EDIT_MATRIX')" in open(os.path.join(ROOT, 'ciri_long_amd', 'collapse.py')).read()


def test_the_collapse_route_follows_the_switch_and_a_substituted_pair_function(monkeypatch):
    from ciri_long_amd import collapse
    monkeypatch.delenv('CLH_NO_EDIT_MATRIX', raising=False)
    assert collapse._grouped_route()
    monkeypatch.setenv('CLH_NO_EDIT_MATRIX', '1')
    assert not collapse._grouped_route()
    monkeypatch.delenv('CLH_NO_EDIT_MATRIX')
    monkeypatch.setattr(collapse, 'distance_batch', lambda xs, ys: [0] * len(xs))
    assert not collapse._grouped_route()
