"""The host side of ciri_long_amd.edlib: getNiceAlignment, CIGAR formatting, argument errors, alphabetLength (the
checker's).  No GPU: argument errors are raised before any device is opened."""
import pytest

import edlib_check
from ciri_long_amd import edlib


def test_cigar_string_from_bam_ops():
    assert edlib.cigar_string([(3 << 4) | 7, (1 << 4) | 1]) == '3=1I'
    assert edlib.cigar_string([(12 << 4) | 8, (2 << 4) | 2, (1 << 4) | 7]) == '12X2D1='
    assert edlib.cigar_string([]) == ''


def test_nice_alignment_of_the_issue_example():
    r = {'editDistance': 1, 'alphabetLength': 5, 'locations': [(1, 3), (1, 4)], 'cigar': '3=1I'}
    assert edlib.getNiceAlignment(r, 'ACTG', 'CACTRT') == {
        'query_aligned': 'ACTG', 'matched_aligned': '|||-', 'target_aligned': 'ACT-'}


def test_nice_alignment_all_ops_and_gap_symbol():
    r = {'editDistance': 3, 'alphabetLength': 4, 'locations': [(2, 7)], 'cigar': '2=1X1D1I2='}
    got = edlib.getNiceAlignment(r, b'ACGTTA', b'GGACTCTAC', gapSymbol='*')
    assert got == {'query_aligned': 'ACG*TTA', 'matched_aligned': '||.**||', 'target_aligned': 'ACTC*TA'}
    assert len(set(map(len, got.values()))) == 1


def test_nice_alignment_needs_a_path():
    with pytest.raises(ValueError):
        edlib.getNiceAlignment({'editDistance': 1, 'alphabetLength': 2, 'locations': [(None, 3)], 'cigar': None}, 'A', 'C')
    with pytest.raises(ValueError):
        edlib.getNiceAlignment({'editDistance': -1, 'alphabetLength': 2, 'locations': [], 'cigar': None}, 'A', 'C')


def test_results_from_rows_formats_each_task():
    import numpy as np
    from ciri_long_amd import hip
    rows = np.zeros(2, dtype=hip.EDIT_ALIGN_DTYPE)
    rows[0] = (1, 2, 0, 0, 2, 0, 5, 0)
    rows[1] = (-1, 0, 2, -1, 0, hip.EA_ST_ABOVE_K, 3, 0)
    locs = np.array([[1, 3], [1, 4]], dtype=np.int32)
    cig = np.array([(3 << 4) | 7, (1 << 4) | 1], dtype=np.uint32)
    got = edlib.results_from_rows(rows, locs, cig, 'path')
    assert got[0] == {'editDistance': 1, 'alphabetLength': 5, 'locations': [(1, 3), (1, 4)], 'cigar': '3=1I'}
    assert got[1] == {'editDistance': -1, 'alphabetLength': 3, 'locations': [], 'cigar': None}
    assert edlib.results_from_rows(rows[:1], locs, cig, 'distance')[0]['locations'] == [(None, 3), (None, 4)]


@pytest.mark.parametrize('kw', [{'mode': 'XX'}, {'mode': 'nw'}, {'task': 'cigar'}, {'task': None},
                                {'additionalEqualities': [('A', 'C', 'G')]}, {'additionalEqualities': [('AB', 'C')]}])
def test_argument_errors(kw):
    with pytest.raises(ValueError):
        edlib.align('ACGT', 'ACGT', **kw)


def test_batch_length_mismatch():
    with pytest.raises(ValueError):
        edlib.align_batch(['A', 'C'], ['A'])
    assert edlib.align_batch([], []) == []


def test_alphabet_length_counts_query_and_target():
    assert edlib_check.align('ACTG', 'CACTRT', 'HW')['alphabetLength'] == 5
    assert edlib_check.align('', '')['alphabetLength'] == 0
    assert edlib_check.align('aA', 'Aa')['alphabetLength'] == 2
    assert edlib_check.align(bytes(range(256)), b'')['alphabetLength'] == 256
    assert edlib_check.align('NNN', 'ACGT', additionalEqualities=[('N', 'A')])['alphabetLength'] == 5


def test_checker_pins_the_documented_edge_answers():
    assert edlib_check.align('', 'ACG', 'SHW', 'path') == {'editDistance': 1, 'alphabetLength': 3, 'locations': [(0, 0)], 'cigar': '1D'}
    assert edlib_check.align('', 'ACG', 'NW', 'path')['cigar'] == '3D'
    assert edlib_check.align('AC', '', 'HW', 'path') == {'editDistance': 2, 'alphabetLength': 2, 'locations': [(0, -1)], 'cigar': '2I'}
    assert edlib_check.align('A', 'C', 'HW', 'locations')['locations'] == [(0, -1), (0, 0)]
