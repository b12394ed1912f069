"""The host arithmetic of the genome-window calls of ssw_wrap (align_windows_ends, _band, _spliced, extend_anchors_genome), against
cases written out by hand: window-relative spans to forward-strand contig coordinates (minus windows and empty spans included), a
spliced CIGAR to its exons, the flanks of an anchor at contig edges, and the refusal of windows outside their contig.  No GPU."""
import pytest

from ciri_long_amd import ssw_wrap


class _Res(object):
    pass


def _res(rb, re_):
    r = _Res()
    r.ref_begin, r.ref_end = rb, re_
    return r


class _Genome(object):
    """what _window_spans reads of a hip.Genome"""
    offset = {'chrA': 0, 'chrB': 1000, 'one': 1500}
    length = {'chrA': 1000, 'chrB': 500, 'one': 1}
    ctx = None


# (start, length, minus, ref_begin, ref_end) -> (genome_begin, genome_end)
COORDS = [
    ((100, 50, False, 0, 49), (100, 149)),        # the whole plus window
    ((100, 50, False, 7, 7), (107, 107)),         # one letter
    ((100, 50, True, 0, 49), (100, 149)),         # the whole minus window: letter 0 is base 149
    ((100, 50, True, 0, 0), (149, 149)),
    ((100, 50, True, 49, 49), (100, 100)),
    ((100, 50, True, 10, 19), (130, 139)),        # genome_begin = start + L - 1 - ref_end = 100 + 49 - 19
    ((0, 1, True, 0, 0), (0, 0)),                 # a contig of one base
    ((100, 50, False, 0, -1), (100, 99)),         # empty spans keep end == begin - 1
    ((100, 50, False, 12, 11), (112, 111)),
    ((100, 50, True, 0, -1), (150, 149)),         # nothing consumed at the start of a minus window: in front of base 149
    ((100, 50, True, 50, 49), (100, 99)),
    ((100, 0, False, 0, -1), (100, 99)),          # a window without a letter
    ((100, 0, True, 0, -1), (100, 99)),
]


@pytest.mark.parametrize('case,want', COORDS)
def test_window_coordinates(case, want):
    start, length, minus, rb, re_ = case
    r = ssw_wrap._window_coords(_res(rb, re_), 'chrA', start, length, minus)
    assert (r.genome_begin, r.genome_end) == want
    assert r.contig == 'chrA' and r.minus is minus
    assert r.genome_end - r.genome_begin == re_ - rb      # the span's length survives, an empty one included


def test_exons_of_spliced_cigars():
    ex = ssw_wrap._exons_of
    assert ex('20M497N20M700N20M', 300) == [(300, 319), (817, 836), (1537, 1556)]
    assert ex('3S20M497N20M5S', 0) == [(0, 19), (517, 536)]                 # soft clips take no reference letter
    assert ex('10M2I10M', 50) == [(50, 69)]                                 # an insertion stays inside its exon
    assert ex('10M3D10M100N5M', 50) == [(50, 72), (173, 177)]               # a deletion too
    assert ex('100N20M', 10) == [(110, 129)]                                # row 0 of an anchored mode as one intron
    assert ex('7N', 10) == [] and ex('4I', 10) == [] and ex('', 10) == [] and ex(None, 10) == []


# (contig length, pos, query_pos, query length, slack, minus) -> (left flank, right flank, first base of the interval)
FLANKS = [
    ((1000, 500, 30, 100, 64, False), (94, 134, 406)),      # room on both sides: query letters + slack
    ((1000, 500, 30, 100, 64, True), (94, 134, 366)),       # minus: the query's left is towards the contig's end: [500 - 134, 500 + 94)
    ((1000, 10, 30, 100, 64, False), (10, 134, 0)),         # the left flank stops at base 0
    ((1000, 10, 30, 100, 64, True), (94, 10, 0)),           # minus: it is the right flank that stops there
    ((1000, 990, 30, 100, 64, False), (94, 10, 896)),       # the right flank stops at the contig's end
    ((1000, 990, 30, 100, 64, True), (10, 134, 856)),
    ((1000, 0, 0, 100, 0, False), (0, 100, 0)),             # an anchor at base 0, no slack
    ((1000, 1000, 100, 100, 0, False), (100, 0, 900)),      # an anchor behind the last base
    ((1000, 0, 0, 100, 8, True), (8, 0, 0)),                # minus at base 0: nothing below pos to extend into
    ((1, 0, 5, 10, 64, False), (0, 1, 0)),                  # a contig of one base
    ((1, 1, 5, 10, 64, True), (0, 1, 0)),
    ((0, 0, 0, 0, 64, False), (0, 0, 0)),
]


@pytest.mark.parametrize('case,want', FLANKS)
def test_anchor_flanks(case, want):
    left, right, start = ssw_wrap._anchor_flanks(*case)
    assert (left, right, start) == want
    ctg_len, pos = case[0], case[1]
    assert 0 <= start and start + left + right <= ctg_len                    # the interval lies in the contig
    assert pos == start + (right if case[5] else left)                       # and the anchor where the flanks meet


def test_windows_outside_their_contig_are_named():
    g = _Genome()
    off, ln = ssw_wrap._window_spans('t', g, [('chrA', 0, 1000), ('chrB', 10, 10), ('one', 0, 1), ('chrB', 499, 500)])
    assert list(off) == [0, 1010, 1500, 1499] and list(ln) == [1000, 0, 1, 1]
    for bad in (('chrA', 0, 1001), ('chrA', -1, 5), ('chrB', 6, 5), ('one', 1, 2), ('nope', 0, 1)):
        with pytest.raises(ValueError) as e:
            ssw_wrap._window_spans('t', g, [('chrA', 0, 1), bad])
        assert 'window 1' in str(e.value) and repr(bad[0]) in str(e.value)
    for call in (lambda: ssw_wrap.align_windows_ends(g, [('chrA', 5, 2000)], [False], ['ACGT']),
                 lambda: ssw_wrap.align_windows_band(g, [('chrA', 5, 2000)], [False], ['ACGT'], 4),
                 lambda: ssw_wrap.align_windows_spliced(g, [('zzz', 5, 20)], ['ACGT']),
                 lambda: ssw_wrap.extend_anchors_genome(g, [('chrA', 1001, 0)], [False], ['ACGT'])):
        with pytest.raises(ValueError):
            call()
