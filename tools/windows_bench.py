"""Pair plans on windows of the resident genome (hip.EndsPlan(windows=...), csrc/genome.hip: genome_gather_kernel) against the route
a caller had before them: slice the contig strings, utils.revcomp, hip.encode, hip.pack, EndsPlan(refs, ref_off).  One process, one
GPU, plan form, the median of R after a warm-up.  Standalone; bench.py is not involved.

  (i)   the gather's HIP-event time and the bytes it moves (every letter read once, written once), beside a hipMemcpyAsync
        device-to-device (torch's Tensor.copy_) of the same letter count in the same process: the ratio gather / memcpy
  (ii)  wall time from coordinates to a ready plan, both routes
  (iii) plan run time (HIP events) of both routes: the same kernels on the same buffer contents, so the two agree within noise; the
        spread (min .. max) of each is printed

Shapes, on a synthetic genome of G bases (soft-masked stretches, N runs):
  (a) N windows of 1-1.5 kb against 1-kb queries, global, half of them on the minus strand
  (b) N / 10 windows of 100 kb against 2-kb queries, spliced, traceback='recompute': create only, (i) and (ii)

Prints one JSON line per shape.
usage: python tools/windows_bench.py [N=20000] [runs=10] [shapes=ab] [G=50000000]"""
import json
import os
import sys
import time

import numpy as np
import torch      # before libclh opens the device (hip._torch_first)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ciri_long_amd import hip, utils  # noqa: E402

ARGS = list(sys.argv[1:])
N = int(ARGS[0]) if len(ARGS) > 0 else 20000
R = int(ARGS[1]) if len(ARGS) > 1 else 10
SHAPES = ARGS[2] if len(ARGS) > 2 else 'ab'
G = int(ARGS[3]) if len(ARGS) > 3 else 50000000


def synthetic_genome(rng, total):
    """two contigs of `total` bases in all: random ACGT, a tenth of it lower case in stretches of 2 kb, an N run per megabase"""
    codes = rng.integers(0, 4, total).astype(np.uint8)
    text = np.frombuffer(b'ACGT', dtype=np.uint8)[codes]
    for s in range(0, total - 2000, 20000):
        text[s:s + 2000] |= 0x20
    for s in range(500000, total - 1000, 1000000):
        text[s:s + 300] = ord('N')
    cut = (total * 3) // 5
    blob = text.tobytes().decode('latin-1')
    return {'chr1': blob[:cut], 'chr2': blob[cut:]}


def memcpy_ms(nbytes, runs):
    """a device-to-device copy of nbytes (Tensor.copy_ between contiguous uint8 tensors of one device: torch issues hipMemcpyAsync,
    device to device), HIP events -> the median of `runs` after a warm-up"""
    src = torch.zeros(nbytes, dtype=torch.uint8, device='cuda'); dst = torch.empty_like(src)
    stream = torch.cuda.current_stream()
    ms = []
    for k in range(runs + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        dst.copy_(src, non_blocking=True)
        e1.record(stream)
        e1.synchronize()
        if k:
            ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))


def med(xs):
    return float(np.median(xs))


def bench(name, ctx, genome, contigs, windows, minus, queries, plan_kw, run_plans):
    mat = hip.score_matrix(2, 2)
    qd, qo = hip.pack([hip.encode(q) for q in queries])
    off = np.array([genome.offset[c] + s for c, s, e in windows], dtype=np.int64)
    ln = np.array([e - s for c, s, e in windows], dtype=np.int64)
    flags = np.where(np.asarray(minus, dtype=bool), 3, 0).astype(np.uint8)

    def windows_route():
        return hip.EndsPlan(ctx, qd, qo, None, None, mat, 3, 1, windows=(genome, off, ln, flags), **plan_kw)

    def strings_route():      # what a caller does today: every window a Python string, reverse-complemented, encoded, packed, uploaded
        refs = []
        for (c, s, e), mn in zip(windows, minus):
            w = contigs[c][s:e]
            refs.append(hip.encode(utils.revcomp(w.upper()) if mn else w))
        rd, ro = hip.pack(refs)
        return hip.EndsPlan(ctx, qd, qo, rd, ro, mat, 3, 1, **plan_kw)

    out = dict(shape=name, windows=len(windows), letters=int(ln.sum()), runs=R)
    wall = {'windows': [], 'strings': []}
    gather = []
    keep = {}
    for k in range(R + 1):
        for route, make in (('windows', windows_route), ('strings', strings_route)):
            t0 = time.perf_counter()
            plan = make()
            dt = (time.perf_counter() - t0) * 1e3
            if k:
                wall[route].append(dt)
                if route == 'windows':
                    gather.append(plan.gather_timing()[0])
            if k == R and run_plans:
                keep[route] = plan
            else:
                plan.close()
    out['create_wall_ms'] = {r: med(v) for r, v in wall.items()}
    out['create_speedup'] = out['create_wall_ms']['strings'] / out['create_wall_ms']['windows']
    moved = 2 * int(ln.sum())
    out['gather_ms'] = med(gather); out['gather_bytes'] = moved; out['gather_GBps'] = moved / med(gather) / 1e6
    cp = memcpy_ms(int(ln.sum()), R)
    out['memcpy_ms'] = cp; out['memcpy_GBps'] = moved / cp / 1e6; out['gather_over_memcpy'] = med(gather) / cp
    if run_plans:
        rows = {}
        for route, plan in keep.items():
            plan.run(); rows[route] = plan.fetch()
            ms = []
            for _ in range(R):
                plan.run(); ms.append(plan.timing())
            out['run_ms_' + route] = dict(median=med(ms), min=float(min(ms)), max=float(max(ms)))
            plan.close()
        same = all(np.array_equal(rows['windows'][0][f], rows['strings'][0][f]) for f in ('score', 'ref_begin', 'ref_end', 'query_begin', 'query_end')) \
            and np.array_equal(rows['windows'][1], rows['strings'][1])
        out['rows_equal'] = bool(same)
    print(json.dumps(out), flush=True)


def main():
    rng = np.random.default_rng(2024)
    contigs = synthetic_genome(rng, G)
    ctx = hip.default_context()
    genome = hip.Genome(ctx, contigs)
    names = list(contigs)

    def place(count, lo, hi):
        wins = []
        for k in range(count):
            c = names[k % 2]
            L = int(rng.integers(lo, hi + 1))
            s = int(rng.integers(0, len(contigs[c]) - L))
            wins.append((c, s, s + L))
        return wins

    def query_from(win, mn, length):
        c, s, e = win
        p = s + int(rng.integers(0, max(1, e - s - length)))
        q = ''.join(ch if ch in 'ACGT' else 'A' for ch in contigs[c][p:p + length].upper())
        return utils.revcomp(q) if mn else q

    if 'a' in SHAPES:
        wins = place(N, 1000, 1500)
        minus = [bool(k & 1) for k in range(N)]
        bench('a', ctx, genome, contigs, wins, minus, [query_from(w, m, 1000) for w, m in zip(wins, minus)], dict(mode='global'), True)
    if 'b' in SHAPES:
        n = max(1, N // 10)
        wins = place(n, 100000, 100000)
        minus = [False] * n
        splice = hip.splice_of('windows_bench', 12, 6)
        bench('b', ctx, genome, contigs, wins, minus, [query_from(w, False, 2000) for w in wins],
              dict(mode='semiglobal', splice=splice, strand=np.ones(n, dtype=np.int8), traceback='recompute'), False)
    genome.close()


if __name__ == '__main__':
    main()
