"""Golden answers for tests/test_oracle_vs_ref.py: every seeded case of that test through the reference's own libssw.so (oracle/_ref,
built from the reference's ssw.c by oracle/Makefile), stored with a CRC-32 of the case so that the test knows it re-made the same inputs.

    python tests/golden/make_oracle_vs_ref_golden.py     (needs oracle/_ref/libssw.so)  -> tests/golden/oracle_vs_ref_golden.json.gz
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
    import test_oracle_vs_ref as t
    if not oracle_lib.have_ref():
        raise SystemExit('oracle/_ref/libssw.so is missing: `make -C oracle ref` where the reference tree is')
    cases = {key: [{'crc': t.case_crc(c), 'want': oracle_lib.ref_align(c[0], c[1], *c[2], **c[3])} for c in cs]
             for key, cs in t.all_cases().items()}
    path = os.path.join(HERE, 'oracle_vs_ref_golden.json.gz')
    with gzip.open(path, 'wt') as f:
        json.dump({'generator': 'tests/golden/make_oracle_vs_ref_golden.py', 'source': "the reference's ssw.c (oracle/_ref/libssw.so)",
                   'cases': cases}, f, separators=(',', ':'))
    print('%s: %d case sets, %d alignments' % (path, len(cases), sum(len(v) for v in cases.values())))


if __name__ == '__main__':
    main()
