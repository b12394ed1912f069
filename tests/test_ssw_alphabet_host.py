"""Alignments over substitution matrices of 6..32 letters, the parts that need no GPU: the CPU oracle against the reference's answers
(tests/golden/ssw_alphabet_golden.json.gz), the refusals of the C ABI that come before any device work, the alphabet encoder and
the BLOSUM62 table of ssw_wrap."""
import ctypes as C
import gzip
import json
import os

import numpy as np
import pytest

from oracle_lib import oracle_align

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'ssw_alphabet_golden.json.gz')


def load_golden():
    with gzip.open(GOLDEN, 'rt') as f:
        return json.load(f)


def golden_codes(g, s):
    lut = np.full(256, -1, dtype=np.int16)
    for i, c in enumerate(g['letters']):
        lut[ord(c)] = i
    return lut[np.frombuffer(s.encode('latin-1'), dtype=np.uint8)].astype(np.int8)


def golden_args(g, c):
    m = np.array(g['matrices'][c['mat']][1], dtype=np.int8)
    return (golden_codes(g, c['ref']), golden_codes(g, c['read'])), dict(
        gap_open=c['gap_open'], gap_extend=c['gap_extend'], flag=c['flag'], score_size=c['score_size'], mat=m,
        maskl=c['mask_len'], filters=c['filters'], filterd=c['filterd'])


def test_golden_covers_the_ground():
    g = load_golden()
    cases = g['cases']
    assert len(cases) >= 500
    edges = {int(round(len(m) ** 0.5)) for _, m in g['matrices']}
    assert {6, 20, 24, 25, 32} <= edges
    assert {c['score_size'] for c in cases} == {0, 1, 2}
    assert set(range(16)) <= {c['flag'] for c in cases}
    assert any(c['mask_len'] < 15 for c in cases) and any(c['mask_len'] >= 15 for c in cases)
    assert max(len(c['read']) for c in cases) >= 4000 and max(len(c['ref']) for c in cases) >= 15000
    assert sum(c['want'] is None for c in cases) >= 10                         # the NULL of score_size 0 on overflow


def test_oracle_equals_golden():
    g = load_golden()
    for k, c in enumerate(g['cases']):
        (ref, read), kw = golden_args(g, c)
        assert oracle_align(ref, read, **kw) == c['want'], k


def test_blosum62_table():
    from ciri_long_amd.ssw_wrap import BLOSUM62, BLOSUM62_ALPHABET
    assert BLOSUM62_ALPHABET == 'ARNDCQEGHILKMFPSTWYVBZX*'
    assert BLOSUM62.shape == (24, 24) and BLOSUM62.dtype == np.int8
    assert (BLOSUM62 == BLOSUM62.T).all()
    ix = BLOSUM62_ALPHABET.index
    assert BLOSUM62[ix('W'), ix('W')] == 11
    assert BLOSUM62[ix('C'), ix('C')] == 9
    assert BLOSUM62[ix('A'), ix('A')] == 4
    assert BLOSUM62[ix('W'), ix('C')] == -2
    assert BLOSUM62[ix('*'), ix('*')] == 1 and BLOSUM62[ix('*'), ix('A')] == -4


def test_encode_alphabet():
    from ciri_long_amd.ssw_wrap import BLOSUM62_ALPHABET, encode_alphabet
    got = encode_alphabet('ARnd*x', BLOSUM62_ALPHABET)
    assert got.dtype == np.int8 and list(got) == [0, 1, 2, 3, 23, 22]
    assert list(encode_alphabet(b'wW', BLOSUM62_ALPHABET)) == [17, 17]
    assert len(encode_alphabet('', BLOSUM62_ALPHABET)) == 0
    with pytest.raises(ValueError):
        encode_alphabet('ARJ', BLOSUM62_ALPHABET)                            # J is not a letter of the alphabet
    assert list(encode_alphabet('ARJo', BLOSUM62_ALPHABET, unknown='X')) == [0, 1, 22, 22]
    with pytest.raises(ValueError):
        encode_alphabet('ARJ', BLOSUM62_ALPHABET, unknown='J')
    with pytest.raises(ValueError):
        encode_alphabet('A', 'A' * 33)


# ---- refusals of the C ABI that come before any device work (libclh.so's plan builder checks the options first) ----------
def _lib():
    from ciri_long_amd import hip
    try:
        return hip.lib()
    except hip.HipUnavailable as e:
        pytest.skip(str(e))


def test_refusals_before_the_device():
    L = _lib()
    # gap_open < gap_extend stays refused for every alphabet, with the existing message, before the edge is looked at
    assert 'gap_open < gap_extend' in _plan_ctx(L, 24, 1, 3)
    assert 'gap_open < gap_extend' in _plan_ctx(L, 40, 1, 3)
    assert 'substitution matrix edge must be 1..32' in _plan_ctx(L, 33, 3, 1)
    assert 'resident genome' in _plan_ctx(L, 24, 3, 1, windows=True)


def _plan_ctx(L, n, gap_open, gap_extend, windows=False):
    """the same refusals through a plan builder that has a (fake, never dereferenced) context: the checks run before it is used"""
    from ciri_long_amd import hip
    mat = np.zeros(n * n, dtype=np.int8)
    o = hip.SswOpts()
    o.mat = mat.ctypes.data; o.n_mat = n; o.gap_open = gap_open; o.gap_extend = gap_extend; o.flag = 1; o.score_size = 2
    o.want_score2 = 1; o.want_cigar = 1
    ro = np.array([0, 4], dtype=np.int64)
    fo = np.array([0, 8], dtype=np.int64)
    fake = C.c_void_p(0x10)
    if windows:
        wl = np.array([8], dtype=np.int32)
        h = L.clh_ssw_plan_windows(fake, 1, ro.ctypes.data, fo.ctypes.data, wl.ctypes.data, None, None, C.byref(o))
    else:
        h = L.clh_ssw_plan(fake, 1, ro.ctypes.data, fo.ctypes.data, None, C.byref(o))
    assert not h
    return hip.last_error()
