"""The pin of ciri_long_amd.edlib against the REAL edlib: tests/golden/edlib_golden.json.gz (tests/golden/make_edlib_golden.py
makes it wherever `pip install edlib` works -- not in the build container, not on the GPU box).

While the file is absent the pin tests SKIP.  The day it is committed they hold the checker (CPU) and the kernels (`-m gpu`) to
edlib on the uniquely defined fields (editDistance, end locations, alphabetLength) and report how often the tie-dependent ones
(HW starts, CIGARs) agree, checking edlib's CIGARs for cost and coverage.  The dry-run test keeps the generator honest today."""
import gzip
import json
import os
import subprocess
import sys

import pytest

import edlib_check

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'edlib_golden.json.gz')
sys.path.insert(0, os.path.join(HERE, 'golden'))


def _load(path):
    with gzip.open(path, 'rt') as f:
        return json.load(f)


def compare(doc, align_batch):
    """align_batch(queries, targets, mode, task) -> [dict].  Asserts the pinned fields; returns {key: (agreeing, total)} for
    the tie-dependent ones (starts, CIGARs)"""
    agree = {}
    qs, ts = [c['query'] for c in doc['cases']], [c['target'] for c in doc['cases']]
    for mode in ('NW', 'SHW', 'HW'):
        for task in ('distance', 'locations', 'path'):
            key = '%s/%s' % (mode, task)
            got = align_batch(qs, ts, mode, task)
            same = 0
            for c, g in zip(doc['cases'], got):
                w = c[key]
                assert g['editDistance'] == w['editDistance'], (key, c['query'], c['target'])
                assert g['alphabetLength'] == w['alphabetLength'], (key, c['query'], c['target'])
                assert [e for _, e in g['locations']] == [e for _, e in w['locations']], (key, c['query'], c['target'])
                wl = [tuple(x) for x in w['locations']]
                if task == 'path' and w['cigar'] is not None:
                    edlib_check.check_invariants({'editDistance': w['editDistance'], 'locations': wl, 'cigar': w['cigar']},
                                                 c['query'], c['target'], mode)
                same += (g['locations'] == [(None if task == 'distance' else s, e) for s, e in wl]) and (g['cigar'] == w['cigar'])
            agree[key] = (same, len(got))
    return agree


def _checker_batch(qs, ts, mode, task):
    return [edlib_check.align(q, t, mode, task) for q, t in zip(qs, ts)]


def _real():
    if not os.path.exists(GOLDEN):
        pytest.skip('tests/golden/edlib_golden.json.gz absent: run tests/golden/make_edlib_golden.py where edlib is installed')
    doc = _load(GOLDEN)
    assert not doc['stub'], 'a stub file is not a pin'
    return doc


def test_checker_against_edlib():
    agree = compare(_real(), _checker_batch)
    print('tie-dependent fields equal to edlib:', agree)


@pytest.mark.gpu
def test_kernels_against_edlib():
    from ciri_long_amd import edlib
    agree = compare(_real(), lambda qs, ts, mode, task: edlib.align_batch(qs, ts, mode, task))
    print('tie-dependent fields equal to edlib:', agree)


STUB = '''
import sys
sys.path.insert(0, %r)
import edlib_check
__version__ = "stub"
def align(query, target, mode="NW", task="distance", k=-1, additionalEqualities=None):
    return edlib_check.align(query, target, mode, task, k, additionalEqualities)
'''


def test_generator_dry_run_with_a_stub(tmp_path):
    (tmp_path / 'edlib.py').write_text(STUB % HERE)
    out = tmp_path / 'g.json.gz'
    subprocess.check_call([sys.executable, os.path.join(HERE, 'golden', 'make_edlib_golden.py'), '--stub', str(tmp_path),
                           '--out', str(out), '--count', '40'])
    doc = _load(str(out))
    assert doc['stub'] and len(doc['cases']) == 40
    agree = compare(doc, _checker_batch)
    assert all(a == b for a, b in agree.values())
    doc['cases'][5]['HW/locations']['editDistance'] += 1           # one altered record is caught
    with pytest.raises(AssertionError):
        compare(doc, _checker_batch)
