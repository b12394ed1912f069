"""Random alignments over substitution matrices of 6..32 letters: the GPU (K1a, csrc/ssw_alpha.hip) against the reference library
(oracle/_ref/libssw.so through tests/oracle_lib.ref_align; the CPU oracle where that build is absent) for <minutes>, printing the
first mismatches and the number of alignments compared.

    timeout -k 10 <seconds> python tools/dev/alphabet_fuzz.py <minutes> [seed]

Every batch draws a matrix edge, a random symmetric matrix (or BLOSUM62), gaps with gap_open >= gap_extend, score_size, flag,
filters and per-alignment maskLen; pairs are mutated copies, unrelated sequences, exact copies that overflow the 8-bit pass and
planted repeats.  Exit status 1 on any mismatch.
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    minutes = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 12345
    import oracle_lib
    from ciri_long_amd import hip
    from ciri_long_amd.ssw_wrap import BLOSUM62
    from test_gpu_ssw_alphabet import as_dict, mutate, random_matrix
    check = oracle_lib.ref_align if oracle_lib.have_ref() else oracle_lib.oracle_align
    ctx = hip.Context(0)
    rng = np.random.default_rng(seed)
    t_end = time.time() + 60.0 * minutes
    cases = batches = bad = 0
    while time.time() < t_end and bad < 10:
        n = int(rng.choice([6, 7, 12, 20, 24, 25, 31, 32]))
        mat = np.ascontiguousarray(BLOSUM62.reshape(-1)) if n == 24 and rng.random() < 0.5 else random_matrix(rng, n)
        gE = int(rng.integers(0, 5)); gO = gE + int(rng.choice([0, 0, 1, 3, 8]))
        score_size = int(rng.choice([0, 1, 2, 2])); flag = int(rng.integers(0, 16))
        filters = int(rng.choice([0, 0, 25, 300])); filterd = int(rng.choice([0, 20, 300, 100000]))
        refs, reads = [], []
        for _ in range(int(rng.integers(20, 200))):
            kind = int(rng.integers(0, 4))
            L = int(rng.choice([1, 3, 15, 16, 17, 40, 128, 300, 700, 1500]))
            R = int(rng.choice([0, 1, 20, 100, 500, 2000, 4000]))
            ref = rng.integers(0, n, R).astype(np.int8)
            if kind == 0 and R > 5:
                a = int(rng.integers(0, max(1, R - L)))
                read = mutate(rng, ref[a:a + L], n, float(rng.choice([0.01, 0.1, 0.3])))
            elif kind == 1:
                read = ref[:L].copy() if R >= L and L > 30 else rng.integers(0, n, L).astype(np.int8)
            elif kind == 2 and R >= 60:
                piece = rng.integers(0, n, min(L, R // 3)).astype(np.int8)
                ref[:len(piece)] = piece; ref[R - len(piece):] = piece
                read = piece
            else:
                read = rng.integers(0, n, L).astype(np.int8)
            if len(read) == 0:
                read = np.zeros(1, dtype=np.int8)
            refs.append(ref); reads.append(read)
        masks = np.array([max(15, len(q) // 2) if rng.random() < 0.7 else int(rng.integers(1, 40)) for q in reads], dtype=np.int32)
        rd, ro = hip.pack(reads); fd, fo = hip.pack(refs)
        rows, cig = ctx.ssw_batch(rd, ro, fd, fo, mat, gO, gE, flag=flag, score_size=score_size, want_score2=True, want_cigar=True,
                                  mask_len=masks, filters=filters, filterd=filterd)
        for k in range(len(reads)):
            got = as_dict(rows[k], cig, len(reads[k]))
            want = check(refs[k], reads[k], gap_open=gO, gap_extend=gE, flag=flag, score_size=score_size, mat=mat, maskl=int(masks[k]),
                         filters=filters, filterd=filterd)
            cases += 1
            if got != want:
                bad += 1
                print('MISMATCH n=%d gaps=%d/%d score_size=%d flag=%d filters=%d filterd=%d maskLen=%d L=%d R=%d\n  gpu  %s\n  want %s'
                      % (n, gO, gE, score_size, flag, filters, filterd, masks[k], len(reads[k]), len(refs[k]), got, want), flush=True)
                if bad >= 10:
                    break
        batches += 1
    ctx.close()
    print('alphabet_fuzz: %d alignments in %d batches, %d mismatches (checker: %s)'
          % (cases, batches, bad, 'reference libssw.so' if check is oracle_lib.ref_align else 'CPU oracle'))
    sys.exit(1 if bad else 0)


if __name__ == '__main__':
    main()
