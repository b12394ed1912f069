"""K7j (csrc/seed_junction.hip): back-splice junctions refined to the base, timed with the HIP events libclh records around the kernels
alone (clh_seed_junction_batch's kernel_ms), the median of R runs after a warm-up.  Standalone; bench.py is not involved.

  (a) N tasks with m of about 33 (29..37, what the planted reads of tests/junction_cases.py give between two anchors at k = 15, w = 5),
  (b) N tasks with m = 256,
both at slack 16 over planted back-splices on an iid genome, reads with 5 % errors, half of them on the minus strand.  Per shape: the
median kernel_ms (and the least and greatest of the runs), tasks per second and cells per second with 2 m (m + slack) cells per task (the two sides).  For context, beside
each: K1g's `extend` mode, score only (clh_ends_*), on 2 N pairs of the same m x (m + slack), the nearest existing route with the same
cell count -- its plan's own HIP-event time.  It computes something else (one matrix's best cell, no site costs, no split), so the
ratio says what the junction's cells cost, not which to use.

There is no parent-commit or reference figure for a step that did not exist.
At N = 20 000 shape (a) is a launch of about a tenth of a millisecond, near the floor of what events resolve: N = 200 000 shows the
rate of the kernel itself.
usage: python tools/junction_bench.py [N=20000] [runs=10]"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ciri_long_amd import hip  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 20000
R = int(sys.argv[2]) if len(sys.argv) > 2 else 10
SLACK = 16
CONTIGS, SIZE = 8, 1 << 20


def plant(rng, codes, spans):
    """per span m one read that crosses a back-splice of its contig between two anchors, 5 % substitutions -> (reads, tasks)"""
    reads, tasks = [], []
    for n, m in enumerate(spans):
        c = n % CONTIGS
        t = int(rng.integers(0, m + 1))
        start = int(rng.integers(1000, SIZE // 2))
        end = int(rng.integers(start + 2000, SIZE - 1000))
        q = np.concatenate([codes[c][end - t - 20:end], codes[c][start:start + (m - t) + 20]]).astype(np.int8)
        hit = rng.random(len(q)) < 0.05
        hit[:20] = hit[len(q) - 20:] = False            # the anchors' letters match
        q = np.where(hit, (q + rng.integers(1, 4, len(q))) & 3, q).astype(np.int8)
        minus = n & 1
        reads.append((3 - q[::-1]).astype(np.int8) if minus else q)
        tasks.append((n, minus, c, end - t, 20, start + (m - t), 20 + m, 0))
    return reads, np.array(tasks, dtype=np.int64)


def main():
    ctx = hip.default_context()
    rng = np.random.Generator(np.random.PCG64(20281))
    codes = [rng.integers(0, 4, SIZE).astype(np.int8) for _ in range(CONTIGS)]
    letters = np.frombuffer(b'ACGT', dtype=np.uint8)
    genome = hip.Genome(ctx, [('g%d' % c, letters[v].tobytes().decode('latin-1')) for c, v in enumerate(codes)])
    idx = hip.SeedIndex(genome, k=15, w=5)
    mat = hip.score_matrix(2, 2)
    for label, spans in (('a: m of about 33', rng.integers(29, 38, N)), ('b: m = 256', np.full(N, 256))):
        reads, tasks = plant(rng, codes, [int(m) for m in spans])
        packed = hip.pack(reads)
        rows = idx.junctions(packed, tasks, slack=SLACK)          # warm-up
        ms = []
        for _ in range(R):
            idx.junctions(packed, tasks, slack=SLACK)
            ms.append(idx.last_junction_ms)
        lo, hi, ms = float(min(ms)), float(max(ms)), float(np.median(ms))
        cells = float(sum(2 * int(m) * (int(m) + SLACK) for m in spans))
        assert (rows[:, 0] == 0).all()
        # K1g extend, score only: two pairs per task of m x (m + slack), the letters the two sides read
        qs, rs = [], []
        for (n, minus, c, xd, yd, xa, ya, _), read in zip(tasks.tolist(), reads):
            s = (3 - read[::-1]).astype(np.int8) if minus else read
            m = ya - yd
            qs += [s[yd:ya], s[yd:ya][::-1]]
            rs += [codes[c][xd:xd + m + SLACK], codes[c][xa - m - SLACK:xa][::-1]]
        (qd, qo), (rd, ro) = hip.pack(qs), hip.pack(rs)
        plan = ctx.ends_plan(qd, qo, rd, ro, mat, 3, 1, mode='extend', want_cigar=False)
        plan.run()
        ref = []
        for _ in range(R):
            plan.run()
            ref.append(plan.timing())
        plan.close()
        ref = float(np.median(ref))
        print(json.dumps({'shape': label, 'tasks': len(tasks), 'slack': SLACK, 'runs': R, 'kernel_ms': round(ms, 4), 'kernel_ms_min_max': [round(lo, 4), round(hi, 4)], 'tasks_per_s': round(len(tasks) / ms * 1e3),
                          'gcells_per_s': round(cells / ms / 1e6, 2), 'k1g_extend_pairs': len(qs),
                          'k1g_extend_ms': round(ref, 4), 'k1g_extend_gcells_per_s': round(cells / ref / 1e6, 2)}), flush=True)
    idx.close()
    genome.close()


if __name__ == '__main__':
    main()
