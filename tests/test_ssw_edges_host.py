"""The CPU statement of the reference's Smith-Waterman (oracle/ssw_oracle.c) at the edges of tests/ssw_edges.py -- the 16-bit score
ceiling, gap extensions above 16, general matrices, score_size 1 / 2, flag 0 / 1 -- against the reference's own answers stored in
tests/golden/ssw_edges_golden.json.gz.  Where oracle/_ref/libssw.so is built, the reference library must give the stored answers too.
tests/test_gpu_ssw_edges.py holds the kernels to the same statement."""
import gzip
import json
import os

import pytest

import ssw_edges
from oracle_lib import have_ref, oracle_align, ref_align

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', ssw_edges.GOLDEN_NAME)
KEYS = list(ssw_edges.all_cases())


def golden():
    with gzip.open(GOLDEN, 'rt') as f:
        return json.load(f)['cases']


@pytest.mark.parametrize('key', KEYS)
def test_oracle_equals_the_reference_at_the_edges(key):
    cases = ssw_edges.all_cases()[key]
    want = golden()[key]
    assert len(want) == len(cases), key
    for k, (case, w) in enumerate(zip(cases, want)):
        assert ssw_edges.case_crc(case) == w['crc'], 'case %d of %s is not the one the golden file was made from' % (k, key)
        args, kw = ssw_edges.call_args(case)
        assert oracle_align(*args, **kw) == w['want'], (key, k)
        if have_ref():
            assert ref_align(*args, **kw) == w['want'], ('the reference library disagrees with the golden file', key, k)


def test_the_edges_are_reached():
    """the case sets do reach what they are named for: saturated scores (32767) in every ceiling set, scores just below it, the 8-bit
    limit crossed, a non-zero N row in some 5 x 5 matrices"""
    g = golden()
    for key in ('ceiling 10/4/8/2', 'ceiling 10/4/6/6', 'ceiling long', 'ceiling match 1'):
        assert any(w['want']['score'] == 32767 for w in g[key]), key
    assert any(32000 <= w['want']['score'] < 32767 for w in g['ceiling 10/4/8/2'])
    assert any(w['want']['score'] < 32000 for w in g['ceiling 10/4/8/2'])
    assert any(w['want']['score'] < 255 for w in g['score_size and flag']) and any(w['want']['score'] >= 255 for w in g['score_size and flag'])
    mats = [c[3]['mat'] for c in ssw_edges.all_cases()['matrices']]
    assert any(len(m) == 25 and any(m[20:]) for m in mats) and any(len(m) == 25 and not any(m[20:]) for m in mats)
    assert {len(m) for m in mats} == {1, 4, 9, 16, 25}
    assert any(m[1] != m[5] for m in mats if len(m) == 25)        # asymmetric
