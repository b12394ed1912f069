"""K7c (csrc/seed_circle.hip): reads to the sample's circles, the route that existed before it against the one device pass.  Standalone;
bench.py is not involved.

Planted as tools/junction_bench.py plants: an iid genome of 8 x 1 Mb and N one-copy circle reads (a circle of 300..1200 letters, begun
anywhere in it) with 5 % substitutions, half of them given on the minus strand.  For each route the median wall time of R runs after a
warm-up (a host clock around calls that end in a device synchronise), the two routes alternating inside one loop:

  old   seed.call_circles: link_reads with every row back on the host, paths and tasks built in Python, the reads uploaded again for
        clh_seed_junction_batch, Genome.letters for the flanks, a Python loop for the dicts
  new   seed.call_circles_batch up to its arrays (SeedIndex.circles): one upload, one row of 16 words per read and the table back
and beside them the three kernel_ms of the new call (HIP events: select and task build, the junction kernels, finalise and table) and
the five slots of SeedIndex.timing() after it.  The two routes are asserted to name the same circles, read by read.

usage: python tools/circle_bench.py [N=20000] [runs=5]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ciri_long_amd import hip, seed  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 20000
R = int(sys.argv[2]) if len(sys.argv) > 2 else 5
CONTIGS, SIZE = 8, 1 << 20


def plant(rng, codes, n):
    reads = []
    for r in range(n):
        c = r % CONTIGS
        size = int(rng.integers(300, 1201))
        start = int(rng.integers(1000, SIZE - 3000))
        circ = codes[c][start:start + size]
        cut = int(rng.integers(60, size - 60))
        q = np.concatenate([circ[cut:], circ[:cut]]).astype(np.int8)
        hit = rng.random(len(q)) < 0.05
        q = np.where(hit, (q + rng.integers(1, 4, len(q))) & 3, q).astype(np.int8)
        reads.append((3 - q[::-1]).astype(np.int8) if r & 1 else q)
    return reads


def main():
    ctx = hip.default_context()
    rng = np.random.Generator(np.random.PCG64(20291))
    codes = [rng.integers(0, 4, SIZE).astype(np.int8) for _ in range(CONTIGS)]
    letters = np.frombuffer(b'ACGT', dtype=np.uint8)
    genome = hip.Genome(ctx, [('g%d' % c, letters[v].tobytes().decode('latin-1')) for c, v in enumerate(codes)])
    idx = seed.index(genome, k=15, w=5)
    packed = hip.pack(plant(rng, codes, N))
    old = seed.call_circles(idx, packed)                 # warm-up of either route, and the comparison
    new = idx.circles(packed)
    mine = seed.circle_dicts(idx, new)
    assert len(old) == len(mine) == N
    for r, (a, b) in enumerate(zip(old, mine)):
        assert ({k: v for k, v in a.items() if k != 'path'} if a else None) == b, r
    wall = {'old': [], 'new': []}
    kernel = []
    for _ in range(R):
        t = time.perf_counter()
        seed.call_circles(idx, packed)
        wall['old'].append(time.perf_counter() - t)
        t = time.perf_counter()
        got = idx.circles(packed)
        wall['new'].append(time.perf_counter() - t)
        kernel.append(got['kernel_ms'])
    timing = idx.timing()
    t_old, t_new = float(np.median(wall['old'])), float(np.median(wall['new']))
    k = np.median(np.array(kernel), axis=0)
    print(json.dumps({'reads': N, 'letters': int(packed[1][-1]), 'runs': R, 'circles_found': sum(1 for b in mine if b), 'table_rows': int(len(new['table'])),
                      'old_call_circles_s': round(t_old, 4), 'old_min_max_s': [round(min(wall['old']), 4), round(max(wall['old']), 4)],
                      'new_circles_s': round(t_new, 4), 'new_min_max_s': [round(min(wall['new']), 4), round(max(wall['new']), 4)],
                      'ratio_old_over_new': round(t_old / t_new, 2), 'kernel_ms_select': round(float(k[0]), 4), 'kernel_ms_junction': round(float(k[1]), 4),
                      'kernel_ms_finalise_table': round(float(k[2]), 4), 'seeds_ms': round(timing['seeds'], 3), 'chain_ms': round(timing['chain'], 3),
                      'link_ms': round(timing['link'], 3), 'shares': idx.info()['shares']}), flush=True)
    idx.close()
    genome.close()


if __name__ == '__main__':
    main()
