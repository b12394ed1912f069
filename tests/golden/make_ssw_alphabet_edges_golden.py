"""Golden answers for tests/test_ssw_alphabet_edges_host.py and tests/test_gpu_ssw_alphabet_edges.py: every seeded case of
tests/ssw_alphabet_edges.py (substitution matrices of 6..32 letters) through the reference's own libssw.so (oracle/_ref, built from the
reference's ssw.c by oracle/Makefile), stored with a CRC-32 of the case so that the tests know they re-made the same inputs.  The file
holds the CRCs and the answers only; the large batches of that module (global_many, pool_pressure) are checked against the CPU oracle.

    python tests/golden/make_ssw_alphabet_edges_golden.py     (needs oracle/_ref/libssw.so)  -> tests/golden/ssw_alphabet_edges_golden.json.gz
"""
import gzip
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    import oracle_lib
    import ssw_alphabet_edges as ssw_edges
    if not oracle_lib.have_ref():
        raise SystemExit('oracle/_ref/libssw.so is missing: `make -C oracle ref` where the reference tree is')
    cases = {}
    for key, cs in ssw_edges.all_cases().items():
        out = []
        for c in cs:
            args, kw = ssw_edges.call_args(c)
            out.append({'crc': ssw_edges.case_crc(c), 'want': oracle_lib.ref_align(*args, **kw)})
        cases[key] = out
    path = os.path.join(HERE, ssw_edges.GOLDEN_NAME)
    # mtime=0: the same cases give the same bytes
    with open(path, 'wb') as raw, gzip.GzipFile(filename='', mode='wb', fileobj=raw, mtime=0) as gz:
        gz.write(json.dumps({'generator': 'tests/golden/make_ssw_alphabet_edges_golden.py', 'source': "the reference's ssw.c (oracle/_ref/libssw.so)",
                             'cases': cases}, separators=(',', ':')).encode())
    print('%s: %d case sets, %d alignments' % (path, len(cases), sum(len(v) for v in cases.values())))


if __name__ == '__main__':
    main()
