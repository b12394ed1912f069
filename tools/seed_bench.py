"""K7 (csrc/seed.hip): the minimizer index of a resident genome, seeds and chains, timed with the HIP events libclh records around
its own device work (SeedIndex.timing), the median of R runs after a warm-up.  Standalone; bench.py is not involved.

  (a) index build of an iid genome of G Mb in 8 contigs at k = 15, w = 5: sketch (count pass, scan, fill pass; the interval holds the one
      read-back of the total between the passes) and sort (rocPRIM's radix sort on the 2k key bits) apart.  The bound it is to be read
      against is printed beside it: the bytes the sketch must move -- 1 B per base read by each pass, 16 B per entry written -- at the
      HBM rate given with --hbm (GB/s, default 4000, the copy rate DESIGN.md section 3 measures).
  (b) seeds of N reads of about 1 kb cut from the genome, odd ones reverse-complemented, mutated at 10 %: sketch of the reads, look-up,
      scan, anchor fill and the two sorts; no transfer to the host is in the interval.  Anchors per second, and the look-ups per second
      (two binary searches of log2(entries) dependent loads each).
  (c) chains of the same reads: the seeds step again, and the chain kernels apart.
  (d) links of the same reads (clh_seed_link_batch: seeds, chains, and the link kernel behind the chain kernel): the three steps
      apart, and their sum beside what clh_seed_chain_batch takes on the same reads with the same chain options (max_chains 32) -- the
      one figure the link step has a predecessor for.  The link slot is the kernel alone; the marker fill of its rows is outside it.  Linear reads give one chain each, so the link kernel's work here is its floor: header, rank
      and one extraction per segment.

There is no parent-commit or reference figure for a step that did not exist: no ratio is printed.
usage: python tools/seed_bench.py [G=100] [N=100000] [runs=10] [shapes=abcd] [--hbm GBPS]"""
import json
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ciri_long_amd import hip, synth  # noqa: E402

ARGS = list(sys.argv[1:])
HBM = 4000.0
if '--hbm' in ARGS:
    at = ARGS.index('--hbm')
    HBM = float(ARGS[at + 1])
    del ARGS[at:at + 2]
G = int(ARGS[0]) if len(ARGS) > 0 else 100
N = int(ARGS[1]) if len(ARGS) > 1 else 100000
R = int(ARGS[2]) if len(ARGS) > 2 else 10
SHAPES = ARGS[3] if len(ARGS) > 3 else 'abcd'
K, W = 15, 5


def main():
    ctx = hip.default_context()
    rng = np.random.Generator(np.random.PCG64(20271))
    per = G * 1000000 // 8
    codes = [rng.integers(0, 4, per).astype(np.int8) for _ in range(8)]
    letters = np.frombuffer(b'ACGT', dtype=np.uint8)
    genome = hip.Genome(ctx, [('g%d' % c, letters[v].tobytes().decode('latin-1')) for c, v in enumerate(codes)])
    idx = hip.SeedIndex(genome, k=K, w=W)               # warm-up (code objects, allocator), and the index of b and c
    info = idx.info()
    if 'a' in SHAPES:
        sk, so = [], []
        for _ in range(R):
            other = hip.SeedIndex(genome, k=K, w=W)
            t = other.timing()
            other.close()
            sk.append(t['sketch']); so.append(t['sort'])
        sk, so = float(np.median(sk)), float(np.median(so))
        moved = 2.0 * 8 * per + 16.0 * info['entries']   # each pass reads every base once; the fill pass writes the entries
        print(json.dumps({'shape': 'a: index build, %d Mb, k %d w %d' % (G, K, W), 'bases': 8 * per, 'entries': info['entries'], 'distinct': info['distinct'],
                          'index_bytes': info['bytes'], 'sketch_ms': round(sk, 3), 'sort_ms': round(so, 3), 'sketch_gbases_per_s': round(8 * per / sk / 1e6, 2),
                          'sketch_bytes_moved': moved, 'sketch_bound_ms_at_%g_GBps' % HBM: round(moved / HBM / 1e6, 3),
                          'sort_entries_per_s': round(info['entries'] / so * 1e3)}), flush=True)
    if 'b' in SHAPES or 'c' in SHAPES or 'd' in SHAPES:
        reads = []
        for r in range(N):
            v = codes[r % 8]
            L = int(rng.integers(800, 1201))
            a = int(rng.integers(0, per - L))
            q = synth.mutate(v[a:a + L], rng, sub=0.04, ins=0.03, dele=0.03)
            reads.append((3 - q[::-1]).astype(np.int8) if r & 1 else q)
        packed = hip.pack(reads)
        nmin = sum(len(p) for p, _, _ in idx.minimizers(packed))
        got = idx.seeds(packed)                         # warm-up
        anchors = int(got['anchor_off'][-1])
        if 'b' in SHAPES:
            ms = []
            for _ in range(R):
                idx.seeds(packed)
                ms.append(idx.timing()['seeds'])
            ms = float(np.median(ms))
            print(json.dumps({'shape': 'b: seeds, %d reads of about 1 kb at 10 %% error' % N, 'letters': int(packed[1][-1]), 'minimizers': nmin, 'anchors': anchors,
                              'repetitive': int(got['repetitive'].sum()), 'shares': idx.info()['shares'], 'seeds_ms': round(ms, 3),
                              'reads_per_s': round(N / ms * 1e3), 'anchors_per_s': round(anchors / ms * 1e3), 'lookups_per_s': round(nmin / ms * 1e3),
                              'dependent_loads_per_lookup': 2 * int(math.ceil(math.log2(max(info['entries'], 2))))}), flush=True)
        if 'c' in SHAPES:
            chains, _ = idx.chains(packed)              # warm-up
            ms, se = [], []
            for _ in range(R):
                idx.chains(packed)
                t = idx.timing()
                ms.append(t['chain']); se.append(t['seeds'])
            ms, se = float(np.median(ms)), float(np.median(se))
            print(json.dumps({'shape': 'c: chains of the same reads, defaults', 'anchors': anchors, 'chains': sum(len(c) for c in chains),
                              'reads_with_a_chain': sum(1 for c in chains if c), 'seeds_ms': round(se, 3), 'chain_ms': round(ms, 3),
                              'reads_per_s': round(N / (ms + se) * 1e3), 'chain_anchors_per_s': round(anchors / ms * 1e3)}), flush=True)
        if 'd' in SHAPES:
            got = idx.links(packed)                     # warm-up
            both = {'chain_batch': [], 'link_batch': [], 'link': [], 'chain': [], 'seeds': []}
            for _ in range(R):
                idx.chains(packed, max_chains=32)       # the same chain options as links(): the difference is the link step alone
                t = idx.timing()
                both['chain_batch'].append(t['seeds'] + t['chain'])
                idx.links(packed)
                t = idx.timing()
                both['link_batch'].append(t['seeds'] + t['chain'] + t['link'])
                for name in ('seeds', 'chain', 'link'):
                    both[name].append(t[name])
            med = {name: float(np.median(v)) for name, v in both.items()}
            print(json.dumps({'shape': 'd: links of the same reads, defaults (max_chains 32)', 'segments': 2 * N, 'chains': int(got['seg'][:, 0].sum()),
                              'paths': int(got['link_seg'][:, 1].sum()), 'seeds_ms': round(med['seeds'], 3), 'chain_ms': round(med['chain'], 3),
                              'link_ms': round(med['link'], 3), 'link_batch_ms': round(med['link_batch'], 3),
                              'chain_batch_ms': round(med['chain_batch'], 3), 'segments_per_s': round(2 * N / med['link'] * 1e3)}), flush=True)
    idx.close()
    genome.close()


if __name__ == '__main__':
    main()
