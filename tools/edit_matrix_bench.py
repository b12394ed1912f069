"""Step 1 of collapse.cluster_steps -- the distance matrices of all requests of a round -- at the C5 shape: 100 requests of 50
homopolymer-compressed reads of about 500 letters, 122 500 pairs.  Standalone; bench.py is not involved.

  wall time of the step through the pair route (every pair written out as two strings for clh_edit_distance_batch: the code
  of the commit before the grouped call, kept as collapse._pair_route_matrices) and through the grouped route
  (utils.pairwise_distance_groups over clh_edit_matrix_batch), and of the compression in front of it ([utils.compress_seq] against
  utils.compress_seq_batch);
  HIP-event time of the resident plans: EditMatrixPlan on the compressed strings (task build + K4), on the raw reads with
  hpc=True (compression + task build + K4), and K4 alone on the same pairs (EditPlan).

Prints one JSON line; every time is the median of R runs after a warm-up.  usage: python tools/edit_matrix_bench.py [requests=100] [runs=10]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ciri_long_amd import collapse, hip, synth, utils  # noqa: E402

NREQ = int(sys.argv[1]) if len(sys.argv) > 1 else 100
R = int(sys.argv[2]) if len(sys.argv) > 2 else 10
B = 'ACGT'


def wall(fn):
    res = fn()                                    # warm-up (code objects, allocator)
    ms = []
    for _ in range(R):
        t0 = time.perf_counter()
        res = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), res


def events(plan):
    plan.run(); plan.fetch()
    ms = []
    for _ in range(R):
        plan.run()
        ms.append(plan.timing())
    return float(np.median(ms))


def main():
    ctx = hip.default_context()
    rng = np.random.Generator(np.random.PCG64(synth.SEEDS['C5']))
    raw = []
    for _ in range(NREQ):
        tm = synth.template(rng)
        raw.append([''.join(B[b] for b in synth.mutate(np.roll(tm, int(rng.integers(0, len(tm)))), rng)) for _ in range(50)])
    flat = [s for g in raw for s in g]
    t_hpc_py, hpc_flat = wall(lambda: [utils.compress_seq(s) for s in flat])
    t_hpc_gpu, hpc_gpu = wall(lambda: utils.compress_seq_batch(flat))
    assert hpc_gpu == hpc_flat
    lists = [hpc_flat[k * 50:(k + 1) * 50] for k in range(NREQ)]
    t_pairs, m_pairs = wall(lambda: collapse._pair_route_matrices(lists))
    t_groups, m_groups = wall(lambda: utils.pairwise_distance_groups(lists))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(m_pairs, m_groups))
    xs, ys = [], []
    for g in lists:
        ii, jj = np.triu_indices(len(g), 1)
        xs += [g[i] for i in ii]; ys += [g[j] for j in jj]
    k4 = ctx.edit_plan(xs, ys)
    t_k4 = events(k4)
    k4.close()
    em = ctx.edit_matrix_plan(lists)
    t_em = events(em)
    em.close()
    emh = ctx.edit_matrix_plan(raw, hpc=True)
    t_emh = events(emh)
    emh.close()
    print(json.dumps({'shape': '%d requests x 50 reads' % NREQ, 'pairs': len(xs), 'mean_hpc_len': round(float(np.mean([len(s) for s in hpc_flat])), 1),
                      'runs': R, 'step1_pair_route_wall_ms': round(t_pairs, 3), 'step1_grouped_route_wall_ms': round(t_groups, 3),
                      'step1_speedup': round(t_pairs / t_groups, 2), 'compress_python_wall_ms': round(t_hpc_py, 3),
                      'compress_device_wall_ms': round(t_hpc_gpu, 3), 'k4_pairs_plan_ms': round(t_k4, 4), 'matrix_plan_ms': round(t_em, 4),
                      'matrix_plan_hpc_ms': round(t_emh, 4), 'tasks_over_k4': round(t_em / t_k4, 3), 'hpc_and_tasks_over_k4': round(t_emh / t_k4, 3)}), flush=True)


if __name__ == '__main__':
    main()
