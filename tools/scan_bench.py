"""The row-scan kernels (K1s: csrc/ssw_scan.hip, K1w: csrc/ssw_scan_wide.hip) by launch class: fixed-seed batches, one per class, and per
batch the median over 10 profiled plan runs of the class's kernel time (Plan.timing() by Plan.segments(), the prefilter's own kernel from
Plan.prefilter_timing()).  One JSON line per batch.

    python tools/scan_bench.py                  every batch
    python tools/scan_bench.py --dump DIR       also writes each batch's result rows to DIR/<batch>.npy (two builds must agree byte for byte)
    CLH_LIB=/path/to/libclh.so python tools/scan_bench.py        another build of the library (ciri_long_amd/hip.py)

The batches are sized for tens of milliseconds per run: long enough to time, short enough that two builds can be alternated A B A B A B."""
import argparse
import json
import os
import sys

import numpy as np
import torch                      # before libclh.so is loaded, as in the other tools: torch brings its own HIP runtime

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CLASS = {'kRvScan': 0, 'kRvScanSliced': -1, 'kRvScanWide': -3, 'kRvScanWideSliced': -4, 'kRvScanTr': -9}     # csrc/clh_device.h
RUNS = 10


def _copy(rng, text, L, err):
    """an L-base stretch of text with a fraction err of its bases mutated (a third each: substitution, insertion, deletion)"""
    from ciri_long_amd import synth
    pos = int(rng.integers(0, len(text) - L))
    return synth.mutate(text[pos:pos + L], rng, sub=err / 3, ins=err / 3, dele=err / 3)[:L]


def _pairs(seed, n, read_len, win_len, err, absent=0.25):
    """n (read, window) pairs: the read is a mutated stretch of its window, or (a fraction `absent`) unrelated to it"""
    rng = np.random.Generator(np.random.PCG64([seed, 20]))
    reads, wins = [], []
    for _ in range(n):
        w = rng.integers(0, 4, int(rng.integers(win_len[0], win_len[1] + 1)), dtype=np.int8)
        L = int(rng.integers(read_len[0], min(read_len[1], len(w) - 1) + 1))
        r = rng.integers(0, 4, L, dtype=np.int8) if rng.random() < absent else _copy(rng, w, L, err)
        reads.append(r if len(r) else w[:1].copy()); wins.append(w)
    return reads, wins


def _short_refs(seed, n):
    """kRvScanTr: reads of 300-4000 bases that hold a noisy copy of their reference of 20-64 columns"""
    from ciri_long_amd import synth
    rng = np.random.Generator(np.random.PCG64([seed, 21]))
    reads, refs = [], []
    for _ in range(n):
        ref = rng.integers(0, 4, int(rng.integers(20, 65)), dtype=np.int8)
        q = rng.integers(0, 4, int(rng.integers(300, 4001)), dtype=np.int8)
        core = synth.mutate(ref, rng, sub=0.04, ins=0.03, dele=0.03)
        a = int(rng.integers(0, len(q) - len(core)))
        q[a:a + len(core)] = core
        reads.append(q); refs.append(ref)
    return reads, refs


# (name, class, scheme, builder, copies of what it builds in one plan, environment for the plan).  The copies make a run long enough to
# time without making the batch slow to build; kRvScanTr stays below the 32 768 short references at which the plan sends them to K1l.
BATCHES = [
    ('scan_1111', 'kRvScan', (1, 1, 1, 1), lambda: _pairs(1, 32768, (20, 250), (2000, 2000), 0.06), 8, {}),
    ('scan_1121', 'kRvScan', (1, 1, 2, 1), lambda: _pairs(2, 32768, (20, 250), (2000, 2000), 0.06), 8, {}),
    ('scan_sliced_prefilter', 'kRvScanSliced', (1, 1, 1, 1), lambda: _pairs(3, 256, (20, 250), (40000, 400000), 0.06), 8, {}),
    ('scan_sliced_no_prefilter', 'kRvScanSliced', (1, 1, 1, 1), lambda: _pairs(3, 256, (20, 250), (40000, 400000), 0.06), 8, {'CLH_NO_PREFILTER': '1'}),
    # 1/1/1/1 on ~1 kb reads: unrelated to the window they stay below 255 (byte regime), copies with 4 % errors pass it (word regime,
    # stripe-boundary rows)
    ('wide_1111_byte', 'kRvScanWide', (1, 1, 1, 1), lambda: _pairs(4, 4096, (900, 1100), (2000, 2000), 0.0, absent=1.0), 6, {}),
    ('wide_1111_word', 'kRvScanWide', (1, 1, 1, 1), lambda: _pairs(5, 4096, (900, 1100), (2000, 2000), 0.04, absent=0.0), 6, {}),
    ('wide_10482', 'kRvScanWide', (10, 4, 8, 2), lambda: _pairs(6, 4096, (900, 1100), (2000, 2000), 0.08), 6, {}),
    ('tr_10482', 'kRvScanTr', (10, 4, 8, 2), lambda: _short_refs(7, 8192), 3, {}),
    ('wide_sliced_1111', 'kRvScanWideSliced', (1, 1, 1, 1), lambda: _pairs(8, 128, (300, 2000), (40000, 400000), 0.06), 1, {}),
]


def run_batch(ctx, name, cls, scheme, build, copies, env, dump):
    from ciri_long_amd import hip
    reads, wins = build()
    reads, wins = reads * copies, wins * copies
    rd, ro = hip.pack(reads); fd, fo = hip.pack(wins)
    d_r = torch.from_numpy(rd.view(np.uint8)).cuda(); d_f = torch.from_numpy(fd.view(np.uint8)).cuda()
    m, x, o, e = scheme
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        plan = ctx.plan(ro, fo, hip.score_matrix(m, x), o, e, flag=1, score_size=2, want_score2=False, want_cigar=False)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    segs = plan.segments()
    in_class = sum(c for rv, c, _a, _b in segs if rv == CLASS[cls])
    plan.set_profiling(True)
    st = torch.cuda.current_stream().cuda_stream
    ms, pf = [], []
    for k in range(RUNS + 1):                       # (the first run loads the code objects: not counted)
        plan.run(d_r.data_ptr(), d_f.data_ptr(), st)
        torch.cuda.synchronize()
        k1, _kb = plan.timing()
        if k:
            ms.append(sum(t for (rv, _c, _a, _b), t in zip(segs, k1) if rv == CLASS[cls]))
            pf.append(sum(t for t, _w, _i in plan.prefilter_timing()))
    rows, _ = plan.fetch()
    plan.close()
    if dump:
        np.save(os.path.join(dump, name + '.npy'), rows)
    print(json.dumps({'batch': name, 'class': cls, 'scheme': scheme, 'alignments': len(reads), 'in_class': in_class,
                      'ms_median': round(float(np.median(ms)), 4), 'ms_min': round(min(ms), 4), 'ms_max': round(max(ms), 4),
                      'prefilter_ms_median': round(float(np.median(pf)), 4), 'score_sum': int(rows['score1'].astype(np.int64).sum())}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--dump', metavar='DIR', help='write each batch\'s result rows to DIR/<batch>.npy')
    a = ap.parse_args()
    if a.dump:
        os.makedirs(a.dump, exist_ok=True)
    from ciri_long_amd import hip
    ctx = hip.Context(0)
    for name, cls, scheme, build, copies, env in BATCHES:
        run_batch(ctx, name, cls, scheme, build, copies, env, a.dump)
    ctx.close()


if __name__ == '__main__':
    main()
