"""K4s (csrc/edit_search.hip, edlib.search) against the pair route (K4m, edit_align_plan over the written-out cross product, HW
`locations`) on two shapes, timed with HIP events on the plan form (strings resident, no H2D in the timed run) and with the
host's clock around everything a caller pays: building the lists, the plan (upload), one run, the fetch.  Standalone; bench.py
is not involved.

  (i)  read sets: iid reads of about 1 kb against 8 probes of 20-40 letters on both strands (16 probes per read);
  (ii) long targets: the row "20-200 nt in 1-Mb targets" of tools/edlib_bench.py restricted to probes of at most 64 letters:
       32 mutated copies (10 %) of 20-64-letter pieces of one 1-Mb text, each searched in it.

Prints one JSON line per shape: median ms of R runs for both routes, their ratio, and the wall times.
usage: python tools/edit_search_bench.py [reads=20000] [runs=10]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ciri_long_amd import hip, synth, utils  # noqa: E402

NREADS = int(sys.argv[1]) if len(sys.argv) > 1 else 20000
R = int(sys.argv[2]) if len(sys.argv) > 2 else 10
B = 'ACGT'
_CODE = np.zeros(256, dtype=np.int8)
_CODE[np.frombuffer(B.encode(), dtype=np.uint8)] = np.arange(4)


def text(rng, n):
    return ''.join(B[b] for b in rng.integers(0, 4, n))


def mutate(rng, s, rate):
    codes = _CODE[np.frombuffer(s.encode(), dtype=np.uint8)]
    return ''.join(B[b] for b in synth.mutate(codes, rng, sub=rate / 3, ins=rate / 3, dele=rate / 3))


def timed(plan):
    plan.run(); plan.fetch()                     # warm-up (code objects, allocator)
    ms = []
    for _ in range(R):
        plan.run()
        ms.append(plan.timing())
    return float(np.median(ms))


def wall(make):
    """median wall ms of: build the inputs and the plan, run once, fetch, close"""
    out, res = [], None
    for _ in range(3):
        t0 = time.perf_counter()
        plan = make()
        plan.run()
        res = plan.fetch()
        plan.close()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out)), res


def from_pairs(rows, locs, ntext, nprobe):
    """the pair route's rows as search's five fields"""
    n, at = rows['nlocs'].astype(np.int64), rows['loc_off'].astype(np.int64)
    out = np.zeros(len(rows), dtype=hip.EDIT_SEARCH_DTYPE)
    out['distance'], out['nlocs'] = rows['distance'], rows['nlocs']
    out['start'], out['end'], out['last_end'] = locs[at, 0], locs[at, 1], locs[at + n - 1, 1]
    return out.reshape(ntext, nprobe)


def shape(ctx, name, probes, texts):
    cells = [(t, p) for t in range(len(texts)) for p in range(len(probes))]

    def pair_plan():
        return ctx.edit_align_plan([probes[p] for _, p in cells], [texts[t] for t, _ in cells], 'HW', 'locations')

    def search_plan():
        return ctx.edit_search_plan(probes, texts)
    pl = pair_plan(); pair_ms = timed(pl); pl.close()
    pl = search_plan(); search_ms = timed(pl); info = pl.info(); pl.close()
    pair_wall, (rows, locs, _) = wall(pair_plan)
    search_wall, got = wall(search_plan)
    assert (got == from_pairs(rows, locs, len(texts), len(probes))).all(), 'the two routes disagree'
    print(json.dumps({'shape': name, 'cells': len(cells), 'pair_ms': round(pair_ms, 4),
                      'search_ms': round(search_ms, 4), 'kernel_speedup': round(pair_ms / search_ms, 2), 'pair_wall_ms': round(pair_wall, 2),
                      'search_wall_ms': round(search_wall, 2), 'wall_speedup': round(pair_wall / search_wall, 2), 'seg': info['seg'],
                      'chunks': info['chunks']}), flush=True)


def main():
    ctx = hip.default_context()
    rng = np.random.Generator(np.random.PCG64(synth.SEEDS['C5']))
    # (i)
    probes = []
    for _ in range(8):
        p = text(rng, int(rng.integers(20, 41)))
        probes += [p, utils.revcomp(p)]
    reads = []
    for _ in range(NREADS):
        r = text(rng, int(rng.integers(800, 1201)))
        p = probes[int(rng.integers(0, len(probes)))]
        at = int(rng.integers(0, len(r) - len(p)))
        reads.append(r[:at] + mutate(rng, p, 0.1) + r[at + len(p):])
    shape(ctx, 'i: %d reads of ~1 kb x 8 probes of 20-40 letters, both strands' % NREADS, probes, reads)
    # (ii)
    tlen = 1 << 20
    tg = text(rng, tlen)
    qs = []
    for _ in range(32):
        L = int(rng.integers(20, 61))
        p = int(rng.integers(0, tlen - L))
        qs.append(mutate(rng, tg[p:p + L], 0.1)[:64])
    shape(ctx, 'ii: 32 probes of 20-64 letters in one 1-Mb target', qs, [tg])


if __name__ == '__main__':
    main()
