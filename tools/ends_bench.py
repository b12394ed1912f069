"""K1g (csrc/ssw_ends.hip, end-anchored affine-gap alignment of pairs) against the existing local alignment of the SAME pairs
through clh_ssw_plan (K1w / K1w-T for the DNA shapes, K1a for the proteins), in one process, plan form (sequences resident, no
H2D in the timed run), HIP events, the median of R runs after a warm-up.  Standalone; bench.py is not involved.

  (a) N DNA pairs of 1 kb x 1-1.5 kb, global, score only
  (b) the same with CIGARs
  (c) 1.25 N semiglobal alignments of a 50-nt junction in 2-kb reads under (10, 4, 8, 2), score only
  (d) N BLOSUM62 pairs of 100-500 residues, global, score only (11 / 1)
  (e) 5 000 seed-right flanks of 1 kb x 1 kb -- the query a 10 % mutated copy of the reference for 600 letters, unrelated after --
      in the mode --mode names (default extend), score only; K1g alone, no local run
  (f) the same with CIGARs
  (g) 2 000 spliced pairs -- the query a 600-nt cDNA of three exons mutated at 10 %, the reference a 6-kb window that holds the exons
      around two GT..AG introns of about 2.5 kb -- semiglobal, score only; K1g alone, no local run.  With --splice IO,NC the plan is the
      spliced one (csrc/ssw_ends.hip); without it the same pairs run under one piece or, with --gap2, under two: the yardstick
  (h) the same with CIGARs
  (j) 50 pairs of 20 kb x 20 kb -- the query a 10 % mutated copy of the reference -- global, with CIGARs; K1g alone
  (k) K spliced pairs (--kpairs, default 100) -- a 2-kb cDNA of four exons mutated at 10 % against a 60-kb window that holds them around
      three GT..AG introns of about 15 kb -- semiglobal, with CIGARs; K1g alone.  The workload the recompute route is for.

Prints one JSON line per shape: ms and cells/s (sum of m n over the pairs) of both, and the ratio local / ends of the cell rates.
With CLH_LIB naming another build's libclh.so, `--mode global` times that build on the same pairs: the yardstick of (e) and (f).
--gap2 GO2,GE2 gives every K1g / K1gb plan a second gap piece; --scoring MA,MI,GO,GE replaces 2/2/3/1 in the DNA shapes a, b, e, f
(the long-read costs: --scoring 2,4,4,2 --gap2 24,1); --splice IO,NC gives every K1g plan intron gaps (intron_open, noncanonical).
--traceback stored|recompute names the route to the CIGARs of every K1g plan (default stored; a CLH_LIB build older than the route takes
stored alone); each line then also carries the route, the workspace bytes in use and those of the largest pair.
usage: python tools/ends_bench.py [N=20000] [runs=10] [shapes=abcd] [--mode MODE] [--gap2 GO2,GE2] [--scoring MA,MI,GO,GE] [--splice IO,NC]
                                  [--traceback ROUTE] [--kpairs K]"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from ciri_long_amd import hip, ssw_wrap, synth  # noqa: E402

ARGS = list(sys.argv[1:])
MODE = 'extend'
if '--mode' in ARGS:
    at = ARGS.index('--mode')
    MODE = ARGS[at + 1]
    del ARGS[at:at + 2]
GAP2 = {}                 # --gap2 GO2,GE2: two-piece gap costs (the second piece) for every plan of K1g and K1gb
if '--gap2' in ARGS:
    at = ARGS.index('--gap2')
    GAP2 = dict(zip(('gap_open2', 'gap_extend2'), (int(x) for x in ARGS[at + 1].split(','))))
    del ARGS[at:at + 2]
SPLICE = None             # --splice IO,NC: intron gaps for every plan of K1g (not together with --gap2)
if '--splice' in ARGS:
    at = ARGS.index('--splice')
    SPLICE = tuple(int(x) for x in ARGS[at + 1].split(','))
    del ARGS[at:at + 2]
DNA = (2, 2, 3, 1)        # --scoring MA,MI,GO,GE: match, mismatch and the (first) gap piece of the DNA shapes a, b, e, f
if '--scoring' in ARGS:
    at = ARGS.index('--scoring')
    DNA = tuple(int(x) for x in ARGS[at + 1].split(','))
    del ARGS[at:at + 2]
TRACEBACK = 'stored'      # --traceback stored|recompute: the route to the CIGARs of every K1g plan
if '--traceback' in ARGS:
    at = ARGS.index('--traceback')
    TRACEBACK = ARGS[at + 1]
    del ARGS[at:at + 2]
KPAIRS = 100              # --kpairs K: pairs of shape k
if '--kpairs' in ARGS:
    at = ARGS.index('--kpairs')
    KPAIRS = int(ARGS[at + 1])
    del ARGS[at:at + 2]
N = int(ARGS[0]) if len(ARGS) > 0 else 20000
R = int(ARGS[1]) if len(ARGS) > 1 else 10
SHAPES = ARGS[2] if len(ARGS) > 2 else 'abcd'


def ends_ms(ctx, qd, qo, rd, ro, mat, go, ge, mode, cigar):
    more = dict(splice=hip.splice_of('ends_bench', *SPLICE)) if SPLICE else GAP2
    more = dict(more, traceback=TRACEBACK) if TRACEBACK != 'stored' else more
    plan = ctx.ends_plan(qd, qo, rd, ro, mat, go, ge, mode=mode, want_cigar=cigar, **more)
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


def flanks(rng, count=5000, length=1000, related=600):
    """seed-right flanks: the query is a 10 % mutated copy of the reference's first `related` letters, then unrelated letters"""
    refs = [rng.integers(0, 4, length).astype(np.int8) for _ in range(count)]
    queries = [np.concatenate([synth.mutate(r[:related], rng, sub=0.04, ins=0.03, dele=0.03), rng.integers(0, 4, length).astype(np.int8)])[:length]
               for r in refs]
    return queries, refs


def spliced_pairs(rng, count=2000, exon=200, intron=2500, window=6000, nexons=3):
    """a cDNA of `nexons` exons mutated at 10 % against the window that holds them around GT..AG introns of about `intron` letters"""
    queries, refs = [], []
    for _ in range(count):
        exons = [rng.integers(0, 4, exon).astype(np.int8) for _ in range(nexons)]
        introns = []
        for _ in range(nexons - 1):
            body = rng.integers(0, 4, intron + int(rng.integers(-100, 101))).astype(np.int8)
            body[:2] = (2, 3); body[-2:] = (0, 2)                      # GT .. AG
            introns.append(body)
        core = np.concatenate([x for pair in zip(exons, introns + [exons[0][:0]]) for x in pair])
        flank = max(0, window - len(core))
        refs.append(np.concatenate([rng.integers(0, 4, flank // 2).astype(np.int8), core, rng.integers(0, 4, flank - flank // 2).astype(np.int8)]))
        queries.append(synth.mutate(np.concatenate(exons), rng, sub=0.04, ins=0.03, dele=0.03))
    return queries, refs


def shape(ctx, name, queries, refs, mat, go, ge, mode, cigar, local=True):
    qd, qo = hip.pack(queries); rd, ro = hip.pack(refs)
    cells = float(np.sum(np.diff(qo).astype(np.float64) * np.diff(ro)))
    e_ms, info = ends_ms(ctx, qd, qo, rd, ro, mat, go, ge, mode, cigar)
    if not local:
        print(json.dumps({'shape': name, 'pairs': len(queries), 'cells': cells, 'mode': mode, 'cigar': cigar,
                          'gap2': GAP2 or None, 'splice': SPLICE, 'ends_ms': round(e_ms, 3), 'ends_gcups': round(cells / e_ms / 1e6, 2), 'shares': info['shares'], 'traceback': TRACEBACK,
                          'workspace_bytes': info['workspace_bytes'], 'max_pair_bytes': info['max_pair_bytes']}), flush=True)
        return
    l_ms, classes = local_ms(ctx, qd, qo, rd, ro, mat, go, ge, cigar)
    print(json.dumps({'shape': name, 'pairs': len(queries), 'cells': cells, 'mode': mode, 'cigar': cigar,
                      'gap2': GAP2 or None, 'splice': SPLICE, 'ends_ms': round(e_ms, 3), 'ends_gcups': round(cells / e_ms / 1e6, 2), 'shares': info['shares'],
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
            shape(ctx, 'a: DNA 1 kb x 1-1.5 kb, global, score only', queries, refs, hip.score_matrix(*DNA[:2]), DNA[2], DNA[3], 'global', False)
        if 'b' in SHAPES:
            shape(ctx, 'b: the same with CIGARs', queries, refs, hip.score_matrix(*DNA[:2]), DNA[2], DNA[3], 'global', True)
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
    if 'e' in SHAPES or 'f' in SHAPES:
        queries, refs = flanks(np.random.Generator(np.random.PCG64(20263)))
        if 'e' in SHAPES:
            shape(ctx, 'e: 1-kb seed-right flanks, related for 600 letters, score only', queries, refs, hip.score_matrix(*DNA[:2]), DNA[2], DNA[3], MODE, False, local=False)
        if 'f' in SHAPES:
            shape(ctx, 'f: the same with CIGARs', queries, refs, hip.score_matrix(*DNA[:2]), DNA[2], DNA[3], MODE, True, local=False)
    if 'g' in SHAPES or 'h' in SHAPES:
        queries, refs = spliced_pairs(np.random.Generator(np.random.PCG64(20264)))
        if 'g' in SHAPES:
            shape(ctx, 'g: 600-nt three-exon cDNA x 6-kb window with two introns, semiglobal, score only', queries, refs, hip.score_matrix(*DNA[:2]), DNA[2], DNA[3],
                  'semiglobal', False, local=False)
        if 'h' in SHAPES:
            shape(ctx, 'h: the same with CIGARs', queries, refs, hip.score_matrix(*DNA[:2]), DNA[2], DNA[3], 'semiglobal', True, local=False)
    if 'j' in SHAPES:
        jr = np.random.Generator(np.random.PCG64(20265))
        refs = [jr.integers(0, 4, 20000).astype(np.int8) for _ in range(50)]
        queries = [synth.mutate(r, jr, sub=0.04, ins=0.03, dele=0.03) for r in refs]
        shape(ctx, 'j: 20 kb x 20 kb, global, with CIGARs', queries, refs, hip.score_matrix(*DNA[:2]), DNA[2], DNA[3], 'global', True, local=False)
    if 'k' in SHAPES:
        queries, refs = spliced_pairs(np.random.Generator(np.random.PCG64(20266)), count=KPAIRS, exon=500, intron=15000, window=60000, nexons=4)
        shape(ctx, 'k: 2-kb four-exon cDNA x 60-kb window with three introns, semiglobal, with CIGARs', queries, refs, hip.score_matrix(*DNA[:2]), DNA[2], DNA[3],
              'semiglobal', True, local=False)


if __name__ == '__main__':
    main()
