#!/usr/bin/env python3
"""Golden vectors for ciri_long_amd.edlib from the REAL edlib module (`pip install edlib`; CIRI_long/utils.py:153-159 imports it):

    python tests/golden/make_edlib_golden.py            -> tests/golden/edlib_golden.json.gz   (refuses without the real edlib)

edlib is not installable in the build container or on the GPU box, so its answers are not recorded yet.  Distances, end
locations and alphabetLength are uniquely defined and are held to the plain dynamic programme (tests/edlib_check.py) already;
HW starts and CIGARs follow tie rules, and their parity with edlib is UNPINNED until this file exists.  What it records:
for 600 seeded pairs (DNA, DNA+N, 20 letters; queries of 1..300 letters in targets holding a mutated copy, tandem repeats
or homopolymers; a few empty sides) and every mode x task, edlib.align's dict.  Inputs are stored (they are small).
Under "edges" it records, call by call, the batches of tests/edlib_edges.py all_cases() (lane-group classes, passes, reverse
launches, equalities over eight planes, ...; inputs are named by set and index, not stored -- the sets are seeded).  `--no-edges`
leaves them out; a stub run leaves them out unless `--edges` asks for them (the stand-in would spend minutes on them).
tests/test_edlib_golden.py compares the file with the checker and, with `-m gpu`, with the kernels.

`--stub DIR` puts DIR in front of sys.path first: a directory holding a stand-in `edlib.py`.  That is how the CPU suite dry-runs
this generator (tests/test_edlib_golden.py::test_generator_dry_run_with_a_stub).  A file made that way says `"stub": true`
and is never counted as a pin; it is never written under tests/golden/.
"""
import argparse
import gzip
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, 'edlib_golden.json.gz')
MODES = ('NW', 'SHW', 'HW')
TASKS = ('distance', 'locations', 'path')


def _mutate(rng, s, rate, alpha):
    out = []
    for ch in s:
        r = rng.random()
        if r < rate / 3:
            out.append(rng.choice(alpha))
        elif r < 2 * rate / 3:
            continue
        elif r < rate:
            out += [ch, rng.choice(alpha)]
        else:
            out.append(ch)
    return ''.join(out)


def cases(seed=2026, count=600):
    rng = random.Random(seed)
    out = [('', ''), ('', 'ACGT'), ('ACGT', ''), ('A', 'A'), ('A', 'C'), ('ACTG', 'CACTRT')]
    for i in range(count - len(out)):
        alpha = ('ACGT', 'ACGTN', 'ACDEFGHIKLMNPQRSTVWY')[i % 3]
        m = rng.choice([1, 2, 20, 63, 64, 65, 128, rng.randint(3, 300)])
        kind = i % 4
        if kind == 0:
            unit = ''.join(rng.choice(alpha) for _ in range(rng.randint(1, 6)))
            t = (unit * 400)[:rng.randint(1, 400)]
            q = _mutate(rng, (unit * 300)[:m], rng.choice([0, 0.1, 0.4]), alpha)
        elif kind == 1:
            t = ''.join(rng.choice(alpha) * rng.randint(1, 30) for _ in range(rng.randint(1, 20)))
            q = rng.choice(alpha) * m
        else:
            q = ''.join(rng.choice(alpha) for _ in range(m))
            t = ''.join(rng.choice(alpha) for _ in range(rng.randint(0, 200))) + _mutate(rng, q, rng.choice([0, 0.05, 0.2, 0.4]), alpha) + \
                ''.join(rng.choice(alpha) for _ in range(rng.randint(0, 200)))
        out.append((q or alpha[0], t))
    return out


def edge_calls():
    """-> (set name, batch index, pair index, query, target, mode, task, k, equalities as edlib takes them) for every pair of every
    batch of tests/edlib_edges.py all_cases(), the bounded calls of its k set with their k"""
    sys.path.insert(0, os.path.dirname(HERE))
    import edlib_edges
    for name, batches in edlib_edges.all_cases().items():
        for bi, b in enumerate(batches):
            eq = [(bytes([x]).decode('latin-1'), bytes([y]).decode('latin-1')) for x, y in b.equalities] if b.equalities else None
            for pi, (q, t) in enumerate(zip(b.queries, b.targets)):
                yield name, bi, pi, q, t, b.mode, b.task, b.k, eq


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--edges', action='store_true', help='record the edge sets in a stub run too')
    ap.add_argument('--no-edges', action='store_true', help='leave the edge sets of tests/edlib_edges.py out')
    ap.add_argument('--stub', help='directory with a stand-in edlib.py (dry run; the file is marked as a stub)')
    ap.add_argument('--out', default=OUT)
    ap.add_argument('--count', type=int, default=600)
    a = ap.parse_args(argv)
    if a.stub:
        sys.path.insert(0, a.stub)
        if os.path.abspath(a.out).startswith(HERE + os.sep):
            sys.exit('a stub run never writes under tests/golden/')
    try:
        import edlib
    except ImportError:
        sys.exit('the real edlib module is needed (pip install edlib)')
    recs = []
    for q, t in cases(count=a.count):
        r = {'query': q, 'target': t}
        for mode in MODES:
            for task in TASKS:
                d = edlib.align(q, t, mode=mode, task=task)
                r['%s/%s' % (mode, task)] = {'editDistance': d['editDistance'], 'alphabetLength': d['alphabetLength'],
                                             'locations': [list(x) for x in d['locations']], 'cigar': d.get('cigar')}
        recs.append(r)
    edges = []
    if a.edges or not (a.stub or a.no_edges):
        for name, bi, pi, q, t, mode, task, k, eq in edge_calls():
            d = edlib.align(q, t, mode=mode, task=task, k=k, additionalEqualities=eq)
            edges.append({'set': name, 'batch': bi, 'pair': pi, 'mode': mode, 'task': task, 'k': k, 'editDistance': d['editDistance'],
                          'alphabetLength': d['alphabetLength'], 'locations': [list(x) for x in d['locations']], 'cigar': d.get('cigar')})
    doc = {'stub': bool(a.stub), 'edlib_version': getattr(edlib, '__version__', 'unknown'), 'cases': recs, 'edges': edges}
    with gzip.open(a.out, 'wt') as f:
        json.dump(doc, f)
    print('wrote %d cases to %s' % (len(recs), a.out))


if __name__ == '__main__':
    main()
