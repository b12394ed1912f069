"""Golden answers for alignments over substitution matrices of 6..32 letters: ~600 seeded cases answered by the reference's own
libssw.so (oracle/_ref, built from the reference's ssw.c by oracle/Makefile).  The file holds the inputs and the answers, data only.

    python tests/golden/make_ssw_alphabet_golden.py     (needs oracle/_ref/libssw.so)  -> tests/golden/ssw_alphabet_golden.json.gz

Sequences are stored as letters of LETTERS (code k = LETTERS[k]); matrices as flat lists, row = reference code.  Cases cover
n in {6, 20, 24, 25, 32} with random symmetric matrices and BLOSUM62 (ciri_long_amd.ssw_wrap), reads of 1..5000 letters against
references up to 20000, every score_size, flags 0..15 with score / distance filters, maskLen below and above 15, alignments planted
to overflow the 8-bit pass, and repeats planted so that equal maxima stand far apart (tie rules of score2 / ref_end2).
"""
import gzip
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))

LETTERS = 'ABCDEFGHIJKLMNOPQRSTUVWXYZabcdef'


def random_matrix(rng, n):
    m = rng.integers(-6, 1, size=(n, n))
    m = np.triu(m) + np.triu(m, 1).T
    np.fill_diagonal(m, rng.integers(1, 12, size=n))
    return m.astype(np.int8)


def mutate(rng, s, n, p):
    out = []
    for c in s:
        u = rng.random()
        if u < p / 3:
            continue
        if u < 2 * p / 3:
            out.append(int(rng.integers(n))); continue
        out.append(int(c))
        if u < p:
            out.extend(int(x) for x in rng.integers(0, n, int(rng.integers(1, 6))))
    return np.array(out if out else [0], dtype=np.int8)


def make_cases(seed=20261015, count=600):
    from ciri_long_amd.ssw_wrap import BLOSUM62
    rng = np.random.default_rng(seed)
    mats = [('blosum62', BLOSUM62.astype(np.int8))]
    for n in (6, 20, 24, 25, 32):
        for k in range(2):
            mats.append(('rand%d_%d' % (n, k), random_matrix(rng, n)))
    cases = []
    for ci in range(count):
        mi = int(rng.integers(len(mats)))
        name, m = mats[mi]
        n = m.shape[0]
        kind = ci % 6
        big = ci % 50 == 0                                        # a few long ones: reads up to 5000, references up to 20000
        L = int(rng.integers(1000, 5001)) if big else int(rng.choice([1, 2, 5, 15, 16, 17, 31, 60, 100, 200, 333, 600]))
        R = int(rng.integers(L, 20001)) if big else int(rng.choice([0, 1, 10, 50, 200, 700, 2000]))
        ref = rng.integers(0, n, R).astype(np.int8)
        if kind == 0:                                             # unrelated
            read = rng.integers(0, n, L).astype(np.int8)
        elif kind in (1, 2) and R > 0:                            # a mutated piece of the reference
            a = int(rng.integers(0, max(1, R - L)))
            read = mutate(rng, ref[a:a + L], n, 0.15 if kind == 1 else 0.02)
        elif kind == 3:                                           # planted to overflow the 8-bit pass: a long exact copy
            L = int(rng.integers(60, 400))
            R = max(R, L + 50)
            ref = rng.integers(0, n, R).astype(np.int8)
            a = int(rng.integers(0, R - L))
            read = ref[a:a + L].copy()
        elif kind == 4 and R >= 40:                               # repeats: the same piece twice, far apart -> equal maxima
            L = int(min(L, R // 3)) or 1
            piece = rng.integers(0, n, L).astype(np.int8)
            a = int(rng.integers(0, R // 3 - L + 1)) if R // 3 >= L else 0
            b = int(rng.integers(R // 2, R - L + 1))
            ref[a:a + L] = piece; ref[b:b + L] = piece
            read = piece.copy() if rng.random() < 0.5 else mutate(rng, piece, n, 0.05)
        else:
            read = rng.integers(0, n, L).astype(np.int8)
        if len(read) == 0:
            read = np.zeros(1, dtype=np.int8)
        gE = int(rng.integers(0, 4))
        gO = gE + int(rng.choice([0, 0, 1, 2, 5, 9]))
        flag = int(rng.integers(0, 16))
        score_size = int(rng.choice([0, 1, 2, 2]))
        filters = int(rng.choice([0, 0, 20, 200]))
        filterd = int(rng.choice([0, 10, 100, 100000]))
        maskl = int(rng.choice([5, 14, 15, 16, max(15, len(read) // 2), len(read) // 2]))
        cases.append(dict(mat=mi, read=''.join(LETTERS[c] for c in read), ref=''.join(LETTERS[c] for c in ref), gap_open=gO,
                          gap_extend=gE, flag=flag, score_size=score_size, filters=filters, filterd=filterd, mask_len=maskl))
    return [(name, [int(x) for x in m.reshape(-1)]) for name, m in mats], cases


def decode(s):
    return np.frombuffer(s.encode('latin-1'), dtype=np.uint8).astype(np.int16).copy()


def codes(s):
    lut = np.full(256, -1, dtype=np.int16)
    for i, c in enumerate(LETTERS):
        lut[ord(c)] = i
    return lut[np.frombuffer(s.encode('latin-1'), dtype=np.uint8)].astype(np.int8)


def answer(fn, mats, c):
    m = np.array(mats[c['mat']][1], dtype=np.int8)
    return fn(codes(c['ref']), codes(c['read']), gap_open=c['gap_open'], gap_extend=c['gap_extend'], flag=c['flag'],
              score_size=c['score_size'], mat=m, maskl=c['mask_len'], filters=c['filters'], filterd=c['filterd'])


def main():
    import oracle_lib
    if not oracle_lib.have_ref():
        raise SystemExit('oracle/_ref/libssw.so is missing: `make -C oracle ref` where the reference tree is')
    mats, cases = make_cases()
    for c in cases:
        c['want'] = answer(oracle_lib.ref_align, mats, c)
    path = os.path.join(HERE, 'ssw_alphabet_golden.json.gz')
    with gzip.open(path, 'wt') as f:
        json.dump({'generator': 'tests/golden/make_ssw_alphabet_golden.py', 'source': "the reference's ssw.c (oracle/_ref/libssw.so)",
                   'letters': LETTERS, 'matrices': mats, 'cases': cases}, f, separators=(',', ':'))
    print('%s: %d cases, %d NULL' % (path, len(cases), sum(c['want'] is None for c in cases)))


if __name__ == '__main__':
    main()
