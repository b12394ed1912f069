"""What edlib.search returns for one cell, from tests/edlib_check.py (not a test module): the five fields of
align(probe, text, mode='HW', task='locations'), and the length grids of the edit-search tests."""
import random

import edlib_check

PROBE_LENS = (1, 2, 31, 32, 33, 63, 64)


def expected(probe, text, k=-1, eq=None):
    """(distance, start, end, last_end, nlocs) of edlib_check.align(probe, text, 'HW', 'locations', k, eq), from the functions align
    itself is made of -- with the start of the first location only (align works out one per location)"""
    q, t = edlib_check._arr(probe), edlib_check._arr(text)
    eqm = edlib_check.eq_matrix(eq)
    best, ends = edlib_check.ends_of(q, t, 'HW', eqm)
    if k >= 0 and best > k:
        return (-1, -2, -2, -2, 0)
    return (best, edlib_check.hw_start(q, t, ends[0], best, eqm), ends[0], ends[-1], len(ends))


def text_lens(m, seg):
    """the lengths at which a text of a probe of m letters meets an edge of the scheme with segments of seg columns"""
    return (0, 1, m - 1, m, 2 * m, seg * 64 - 1, seg * 64, seg * 64 + 1, 2 * seg * 64 + 3)


def random_text(rng, n, alpha, probe, plant=True):
    """n letters of alpha, with mutated copies of the probe planted where they fit"""
    t = [rng.choice(alpha) for _ in range(n)]
    m = len(probe)
    if plant and n >= m:
        for _ in range(1 + n // (8 * m + 50)):
            at = rng.randrange(0, n - m + 1)
            for i, c in enumerate(probe):
                t[at + i] = c if rng.random() < 0.9 else rng.choice(alpha)
    return ''.join(t)


def as_tuple(row):
    return tuple(int(row[f]) for f in ('distance', 'start', 'end', 'last_end', 'nlocs'))


def rng_for(*key):
    return random.Random(repr(key))
