"""csrc/edit_search.hip without a GPU: the segment scheme as tools/edit_search_model.py states it -- fresh start per segment,
warm-up walked and not counted, per-segment tuples and their join -- against tests/edlib_check.py, and edlib.search's
argument errors."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import edit_search_model as model  # noqa: E402

import edit_search_check as chk  # noqa: E402


@pytest.mark.parametrize('alpha', ['AC', 'ACGT'])
@pytest.mark.parametrize('seg', [1, 2, 3, 7, 64])
def test_model_equals_the_checker_field_for_field(seg, alpha):
    rng = chk.rng_for('host', seg, alpha)
    for m in chk.PROBE_LENS:
        probe = ''.join(rng.choice(alpha) for _ in range(m))
        for n in chk.text_lens(m, seg):
            text = chk.random_text(rng, n, alpha, probe)
            want = chk.expected(probe, text)
            assert model.search(probe.encode(), text.encode(), seg) == want, (seg, alpha, m, n)
            if want[0] > 0:                                  # the bound at the best and one below it
                assert model.search(probe.encode(), text.encode(), seg, k=want[0]) == want
                assert model.search(probe.encode(), text.encode(), seg, k=want[0] - 1) == (-1, -2, -2, -2, 0)


def test_model_counts_a_run_of_optimal_ends_across_segments_once():
    """a homopolymer probe in a homopolymer text: every column from m - 1 on is an optimal end, whatever the segments are"""
    for seg in (1, 3, 7, 64):
        for m, n in ((5, 200), (33, 64 * seg + 9)):
            got = model.search(b'A' * m, b'A' * n, seg)
            assert got == (0, 0, m - 1, n - 1, n - m + 1) == chk.expected('A' * m, 'A' * n), (seg, m, n)


def test_model_applies_equalities_to_the_letters_as_given():
    eq = [('N', c) for c in 'ACGT']
    probe, text = 'ACNNGT', 'TTACGAGTTTACTTGTAA'
    for seg in (1, 2, 7):
        assert model.search(probe.encode(), text.encode(), seg, eq=[(ord(a), ord(b)) for a, b in eq]) == chk.expected(probe, text, -1, eq)


def test_search_raises_value_error_before_the_library_is_loaded():
    from ciri_long_amd import edlib, hip
    loaded = hip._lib
    for bad in ([('AB', 'C')], [('A',)], [('A', 'B', 'C')], [('', 'A')]):
        with pytest.raises(ValueError):
            edlib.search(['ACGT'], ['ACGTACGT'], additionalEqualities=bad)
    assert hip._lib is loaded
