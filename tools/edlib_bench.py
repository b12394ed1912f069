"""K4m / K4t (csrc/edit_align.hip) on three shapes, timed with HIP events on the plan form (strings resident, no H2D in the
timed run).  Standalone; bench.py is not involved.

  (a) K4's collapse shapes (50 homopolymer-compressed reads per cluster -> 1225 pairs per cluster, tools/collapse_bench.py)
      as NW `distance` through K4m, against K4 on the same pairs.  The shorter string is the query, so both kernels run the
      same blocks over the same columns;
  (b) 20-200-nt queries (mutated copies, 10 %) in 10-kb and in 1-Mb targets, HW `locations` (score pass + reverse passes);
  (c) 1-kb x 1-kb pairs at 5-20 % divergence, NW `path` (score pass + K4t + traceback).

Prints one JSON line per shape: median ms of R runs, forward cells (query x target letters) per second, and for (c) the bytes
K4t stores per cell.  usage: python tools/edlib_bench.py [clusters=100] [runs=10]"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ciri_long_amd import hip, synth, utils  # noqa: E402

NCL = int(sys.argv[1]) if len(sys.argv) > 1 else 100
R = int(sys.argv[2]) if len(sys.argv) > 2 else 10
B = 'ACGT'


def timed(plan):
    plan.run(); plan.fetch()                     # warm-up (code objects, allocator)
    ms = []
    for _ in range(R):
        plan.run()
        ms.append(plan.timing())
    return float(np.median(ms)), plan.fetch()


_CODE = np.zeros(256, dtype=np.int8)
_CODE[np.frombuffer(B.encode(), dtype=np.uint8)] = np.arange(4)


def mutate(rng, s, rate):
    codes = _CODE[np.frombuffer(s.encode(), dtype=np.uint8)]
    return ''.join(B[b] for b in synth.mutate(codes, rng, sub=rate / 3, ins=rate / 3, dele=rate / 3))


def main():
    ctx = hip.default_context()
    rng = np.random.Generator(np.random.PCG64(synth.SEEDS['C5']))
    # (a)
    xs, ys = [], []
    for _ in range(NCL):
        tm = synth.template(rng)
        hpc = [utils.compress_seq(''.join(B[b] for b in synth.mutate(np.roll(tm, int(rng.integers(0, len(tm)))), rng))) for _ in range(50)]
        for i in range(50):
            for j in range(i + 1, 50):
                a, b = (hpc[i], hpc[j]) if len(hpc[i]) <= len(hpc[j]) else (hpc[j], hpc[i])
                xs.append(a); ys.append(b)
    cells = sum(len(a) * len(b) for a, b in zip(xs, ys))
    k4 = ctx.edit_plan(xs, ys)
    t_k4, d_k4 = timed(k4)
    k4m = ctx.edit_align_plan(xs, ys, 'NW', 'distance')
    t_k4m, (rows, _, _) = timed(k4m)
    assert (rows['distance'] == d_k4).all()
    del k4                                       # EditPlan frees its plan when collected
    k4m.close()
    print(json.dumps({'shape': 'a: collapse pairs, NW distance', 'pairs': len(xs), 'cells': cells, 'k4_ms': round(t_k4, 4),
                      'k4m_ms': round(t_k4m, 4), 'k4m_over_k4': round(t_k4m / t_k4, 3), 'k4_cells_per_s': cells / t_k4 * 1e3,
                      'k4m_cells_per_s': cells / t_k4m * 1e3}), flush=True)
    # (b)
    for tlen, npairs in ((10_000, 2000), (1 << 20, 32)):
        tg = ''.join(B[b] for b in rng.integers(0, 4, tlen))
        qs, ts = [], []
        for _ in range(npairs):
            L = int(rng.integers(20, 201))
            p = int(rng.integers(0, tlen - L))
            qs.append(mutate(rng, tg[p:p + L], 0.1)); ts.append(tg)
        cells = sum(len(q) * tlen for q in qs)
        pl = ctx.edit_align_plan(qs, ts, 'HW', 'locations')
        t, (rows, locs, _) = timed(pl)
        pl.close()
        print(json.dumps({'shape': 'b: HW locations, %d-letter targets' % tlen, 'pairs': npairs, 'cells': cells, 'ms': round(t, 4),
                          'cells_per_s': cells / t * 1e3, 'locations': int(len(locs))}), flush=True)
    # (c)
    qs, ts = [], []
    for i in range(4000):
        q = ''.join(B[b] for b in rng.integers(0, 4, 1000))
        qs.append(q); ts.append(mutate(rng, q, (0.05, 0.1, 0.15, 0.2)[i % 4]))
    cells = sum(len(q) * len(t) for q, t in zip(qs, ts))
    stored = sum(20 * ((len(q) + 63) // 64) * len(t) for q, t in zip(qs, ts))
    pl = ctx.edit_align_plan(qs, ts, 'NW', 'path')
    t, _ = timed(pl)
    pl.close()
    print(json.dumps({'shape': 'c: 1 kb x 1 kb, 5-20 % divergence, NW path', 'pairs': len(qs), 'cells': cells, 'ms': round(t, 4),
                      'cells_per_s': cells / t * 1e3, 'stored_bytes_per_cell': round(stored / cells, 4)}), flush=True)


if __name__ == '__main__':
    main()
