"""The CPU statement of the reference's Smith-Waterman (oracle/ssw_oracle.c) over substitution matrices of 6..32 letters at the edges of
tests/ssw_alphabet_edges.py -- asymmetric matrices, the read-length buckets, the 8-bit threshold, the 16-bit ceiling, the traceback's
windows, the gap costs -- against the reference's own answers stored in tests/golden/ssw_alphabet_edges_golden.json.gz.  Where
oracle/_ref/libssw.so is built, the reference library must give the stored answers too.  tests/test_gpu_ssw_alphabet_edges.py holds the
kernels to the same statement."""
import gzip
import json
import os

import numpy as np
import pytest

import ssw_alphabet_edges as edges
from oracle_lib import have_ref, oracle_align, ref_align

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', edges.GOLDEN_NAME)
KEYS = list(edges.all_cases())


def golden():
    with gzip.open(GOLDEN, 'rt') as f:
        return json.load(f)['cases']


@pytest.mark.parametrize('key', KEYS)
def test_oracle_equals_the_reference_at_the_edges(key):
    cases = edges.all_cases()[key]
    want = golden()[key]
    assert len(want) == len(cases), key
    for k, (case, w) in enumerate(zip(cases, want)):
        assert edges.case_crc(case) == w['crc'], 'case %d of %s is not the one the golden file was made from' % (k, key)
        args, kw = edges.call_args(case)
        assert oracle_align(*args, **kw) == w['want'], (key, k)
        if have_ref():
            assert ref_align(*args, **kw) == w['want'], ('the reference library disagrees with the golden file', key, k)


def _bias(mat):
    return -min(0, min(mat))


def test_the_edges_are_reached():
    """the case sets reach what they are named for"""
    g = golden()
    cs = edges.all_cases()
    # the 16-bit ceiling: saturated scores in each form, scores just below it
    ceil = [(c, w['want']) for c, w in zip(cs['ceiling'], g['ceiling'])]
    assert all(w is not None for _c, w in ceil)
    for lo, hi in ((1, 300), (2900, 3700), (8193, 9000)):           # diagonal 127 (LDS), BLOSUM62 W-W, diagonal 4 (global form)
        sub = [w['score'] for c, w in ceil if lo <= len(c[1]) <= hi]
        assert 32767 in sub and any(32700 <= s < 32767 for s in sub), (lo, hi, sorted(set(sub)))
    assert sum(w['score'] == 32766 for _c, w in ceil) >= 4
    # both sides of the 8-bit threshold (score + bias 253..256) for every matrix, NULL exactly where score_size 0 overflows
    by_mat = {}
    for c, w in zip(cs['8-bit threshold'], g['8-bit threshold']):
        by_mat.setdefault(tuple(c[2]), []).append((c[3]['score_size'], None if w['want'] is None else w['want']['score'] + _bias(c[2])))
    assert {(min(m), max(m)) for m in by_mat} == {(lo, hi) for lo in (-1, -6, -128) for hi in (11, 127)}
    for m, got in by_mat.items():
        assert {s for ss, s in got if ss != 0} == {253, 254, 255, 256}, (min(m), max(m))
        assert {s for ss, s in got if ss == 0} == {253, 254, None}, (min(m), max(m))
    # NULLs elsewhere too (score_size 0 in the asymmetric set)
    assert any(w['want'] is None for w in g['asymmetric'])
    # an asymmetric matrix whose transpose would change an answer, in the passes and in the traceback
    diff_score = diff_cigar = 0
    for c in cs['asymmetric']:
        args, kw = edges.call_args(c)
        n = int(round(len(kw['mat']) ** 0.5))
        assert (kw['mat'].reshape(n, n) != kw['mat'].reshape(n, n).T).sum() >= n * (n - 1) // 2
        a = oracle_align(*args, **kw)
        kw['mat'] = np.ascontiguousarray(kw['mat'].reshape(n, n).T.reshape(-1))
        b = oracle_align(*args, **kw)
        if a is None or b is None:
            continue
        diff_score += (a['score'], a['ref_end'], a['query_end']) != (b['score'], b['ref_end'], b['query_end'])
        diff_cigar += a['score'] == b['score'] and a['cigar'] != b['cigar']
    assert diff_score >= 10 and diff_cigar >= 1, (diff_score, diff_cigar)
    # the buckets: every boundary length present
    assert {len(c[1]) for c in cs['buckets']} == set(edges.BUCKET_LENGTHS)
    # the traceback's windows, from the aligned lengths of the reference's answers
    wins = []
    for w in g['traceback windows']:
        w = w['want']
        la, ra = w['query_end'] - w['query_begin'] + 1, w['ref_end'] - w['ref_begin'] + 1
        wins.append((la, ra, abs(ra - la) + 1, len(w['cigar'])))
    bands = {b for _la, _ra, b, _n in wins}
    assert {509, 510, 511, 4093, 4094} <= bands and 255 in bands
    assert any(b in (509, 510, 511) and la + 1 <= edges.SMALL_WS for la, _ra, b, _n in wins)
    assert any(b in (509, 510, 511) and la + 1 > edges.SMALL_WS for la, _ra, b, _n in wins)
    spans = {la + ra for la, ra, _b, _n in wins}
    assert {edges.SMALL_SEQ, edges.SMALL_SEQ + 1, edges.BIG_SEQ, edges.BIG_SEQ + 1} <= spans
    assert any(la + ra > edges.BIG_SEQ and n > 3 for la, ra, _b, n in wins)                    # mutated, unstaged
    assert sum(la + 1 > edges.BIG_WS and b + 3 > edges.BIG_RING for la, _ra, b, _n in wins) >= 2   # the stated CIGAR_TRUNC condition
    # gap costs: gap_open 255, gap_extend 0, gap_open == gap_extend past the 8-bit pass, flags 0 / 1 / 15, masks on both sides of 15
    gc = [(c[3], w['want']) for c, w in zip(cs['gap costs'], g['gap costs'])]
    assert any(kw['gap_open'] == 255 for kw, _w in gc) and any(kw['gap_extend'] == 0 for kw, _w in gc)
    assert any(kw['gap_open'] == kw['gap_extend'] and w['score'] + 4 >= 255 for kw, w in gc)
    assert {kw['flag'] for kw, _w in gc} == {0, 1, 15}
    assert any(kw['maskl'] < 15 for kw, _w in gc) and any(kw['maskl'] >= 15 for kw, _w in gc)
