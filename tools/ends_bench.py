"""K1g (csrc/ssw_ends.hip, end-anchored affine-gap alignment of pairs) against the existing local alignment of the SAME pairs
through clh_ssw_plan (K1w / K1w-T for the DNA shapes, K1a for the proteins), in one process, plan form (sequences resident, no
H2D in the timed run), HIP events, the median of R runs after a warm-up.  Standalone; bench.py is not involved.

  (a) N DNA pairs of 1 kb x 1-1.5 kb, global, score only
  (b) the same with CIGARs
  (c) 1.25 N semiglobal alignments of a 50-nt junction in 2-kb reads under (10, 4, 8, 2), score only
  (d) N BLOSUM62 pairs of 100-500 residues, global, score only (11 / 1)

Prints one JSON line per shape: ms and cells/s (sum of m n over the pairs) of both, and the ratio local / ends of the cell rates.
usage: python tools/ends_bench.py [N=20000] [runs=10] [shapes=abcd]"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from ciri_long_amd import hip, ssw_wrap, synth  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 20000
R = int(sys.argv[2]) if len(sys.argv) > 2 else 10
SHAPES = sys.argv[3] if len(sys.argv) > 3 else 'abcd'


def ends_ms(ctx, qd, qo, rd, ro, mat, go, ge, mode, cigar):
    plan = ctx.ends_plan(qd, qo, rd, ro, mat, go, ge, mode=mode, want_cigar=cigar)
    try:
        plan.run(); plan.fetch()                     # warm-up (code objects, allocator), and the rows are whole
        ms = []
        for _ in range(R):
            plan.run()
            ms.append(plan.timing())
        return float(np.median(ms)), plan.info()
    finally:
        plan.close()


def local_ms(ctx, qd, qo, rd, ro, mat, go, ge, cigar):
    d_q = torch.from_numpy(qd.view(np.uint8)).cuda(); d_r = torch.from_numpy(rd.view(np.uint8)).cuda()
    plan = ctx.plan(qo, ro, mat, go, ge, flag=1, score_size=2, want_score2=False, want_cigar=cigar)
    st = torch.cuda.current_stream().cuda_stream
    try:
        plan.run(d_q.data_ptr(), d_r.data_ptr(), st); plan.fetch()
        ms = []
        for _ in range(R):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            plan.run(d_q.data_ptr(), d_r.data_ptr(), st)
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        classes = sorted(set(s[0] for s in plan.segments()))
        return float(np.median(ms)), classes
    finally:
        plan.close()


def shape(ctx, name, queries, refs, mat, go, ge, mode, cigar):
    qd, qo = hip.pack(queries); rd, ro = hip.pack(refs)
    cells = float(np.sum(np.diff(qo).astype(np.float64) * np.diff(ro)))
    e_ms, info = ends_ms(ctx, qd, qo, rd, ro, mat, go, ge, mode, cigar)
    l_ms, classes = local_ms(ctx, qd, qo, rd, ro, mat, go, ge, cigar)
    print(json.dumps({'shape': name, 'pairs': len(queries), 'cells': cells, 'mode': mode, 'cigar': cigar,
                      'ends_ms': round(e_ms, 3), 'ends_gcups': round(cells / e_ms / 1e6, 2), 'shares': info['shares'],
                      'local_ms': round(l_ms, 3), 'local_gcups': round(cells / l_ms / 1e6, 2), 'local_classes': classes,
                      'local_over_ends': round(e_ms / l_ms, 2)}), flush=True)


def main():
    ctx = hip.default_context()
    rng = np.random.Generator(np.random.PCG64(20261))
    if 'a' in SHAPES or 'b' in SHAPES:
        refs = [rng.integers(0, 4, int(rng.integers(1000, 1501))).astype(np.int8) for _ in range(N)]
        queries = []
        for r in refs:
            at = int(rng.integers(0, len(r) - 999))
            q = synth.mutate(r[at:at + 1000], rng, sub=0.04, ins=0.03, dele=0.03)
            queries.append(np.concatenate([q, rng.integers(0, 4, 1000).astype(np.int8)])[:1000])
        if 'a' in SHAPES:
            shape(ctx, 'a: DNA 1 kb x 1-1.5 kb, global, score only', queries, refs, hip.score_matrix(2, 2), 3, 1, 'global', False)
        if 'b' in SHAPES:
            shape(ctx, 'b: the same with CIGARs', queries, refs, hip.score_matrix(2, 2), 3, 1, 'global', True)
    if 'c' in SHAPES:
        n = N + N // 4
        refs = [rng.integers(0, 4, 2000).astype(np.int8) for _ in range(n)]
        queries = []
        for r in refs:
            at = int(rng.integers(0, 1950))
            q = synth.mutate(r[at:at + 50], rng, sub=0.04, ins=0.03, dele=0.03)
            queries.append(np.concatenate([q, rng.integers(0, 4, 50).astype(np.int8)])[:50])
        shape(ctx, 'c: 50-nt junction in 2-kb reads, semiglobal, 10/4/8/2', queries, refs, hip.score_matrix(10, 4), 8, 2, 'semiglobal', False)
    if 'd' in SHAPES:
        refs = [rng.integers(0, 20, int(rng.integers(100, 501))).astype(np.int8) for _ in range(N)]
        queries = [rng.integers(0, 20, int(rng.integers(100, 501))).astype(np.int8) for _ in range(N)]
        shape(ctx, 'd: BLOSUM62 100-500 residues, global, 11/1', queries, refs, ssw_wrap.BLOSUM62.reshape(-1), 11, 1, 'global', False)


if __name__ == '__main__':
    main()
