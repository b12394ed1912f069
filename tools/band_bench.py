"""K1gb (csrc/ssw_band.hip, banded end-anchored alignment of pairs) against K1g's full matrix (csrc/ssw_ends.hip) on the SAME pairs
through clh_ends_plan, in one process, plan form (sequences resident, no H2D in the timed run), HIP events, the median of R runs
after a warm-up.  Standalone; bench.py is not involved.  In the same run every row with exact == 1 is asserted equal to K1g's row
(and CIGAR, where both were made).

  (a) N DNA pairs of 1 kb against 10 % mutated copies, global, score only, w = 32 / 64 / 128
  (b) the same with CIGARs; the number of workspace shares of each route is printed
  (c) 1.25 N semiglobal placements of a 50-nt junction in 2-kb reads under (10, 4, 8, 2), the true diagonal as hint, w = 16
  (d) N / 100 pairs of 20 kb x 20 kb with CIGARs, w = 128 (K1g stores 200 MB of decisions per pair here)
  (e) 5 000 seed-right flanks of 1 kb x 1 kb -- the query a 10 % mutated copy of the reference for 600 letters, unrelated after --
      in the mode --mode names (default extend), score only, w = 64
  (f) the same with CIGARs

Prints one JSON line per shape and width: ms of both, cells of both (sum of m B against sum of m n), the cell rates, full / band.
With CLH_LIB naming another build's libclh.so, `--mode global` times that build on the same pairs: the yardstick of (e) and (f).
--gap2 GO2,GE2 gives every K1g / K1gb plan a second gap piece; --scoring MA,MI,GO,GE replaces 2/2/3/1 in the DNA shapes a, b, e, f
(the long-read costs: --scoring 2,4,4,2 --gap2 24,1).
usage: python tools/band_bench.py [N=20000] [runs=10] [shapes=abcd] [--mode MODE] [--gap2 GO2,GE2] [--scoring MA,MI,GO,GE]"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ciri_long_amd import hip, synth  # noqa: E402

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
DNA = (2, 2, 3, 1)        # --scoring MA,MI,GO,GE: match, mismatch and the (first) gap piece of the DNA shapes a, b, e, f
if '--scoring' in ARGS:
    at = ARGS.index('--scoring')
    DNA = tuple(int(x) for x in ARGS[at + 1].split(','))
    del ARGS[at:at + 2]
N = int(ARGS[0]) if len(ARGS) > 0 else 20000
R = int(ARGS[1]) if len(ARGS) > 1 else 10
SHAPES = ARGS[2] if len(ARGS) > 2 else 'abcd'


def timed(plan):
    try:
        plan.run(); rows, cig = plan.fetch()         # warm-up (code objects, allocator), and the rows are whole
        ms = []
        for _ in range(R):
            plan.run()
            ms.append(plan.timing())
        return float(np.median(ms)), plan.info(), rows, cig
    finally:
        plan.close()


def same_rows(b_rows, b_cig, e_rows, e_cig, cigar, mode):
    """rows the band certifies equal K1g's -> how many were certified"""
    sel = np.nonzero(b_rows['exact'] == 1)[0]
    fields = ['score', 'ref_end', 'query_end'] + (['ref_begin', 'query_begin', 'cigar_len'] if cigar else [])
    for f in fields:
        assert np.array_equal(b_rows[f][sel], e_rows[f][sel]), f
    if cigar:
        for k in sel:
            a, b = b_rows[k], e_rows[k]
            assert np.array_equal(b_cig[a['cigar_off']:a['cigar_off'] + a['cigar_len']], e_cig[b['cigar_off']:b['cigar_off'] + b['cigar_len']]), k
    return int(len(sel))


def shape(ctx, name, queries, refs, mat, go, ge, mode, cigar, widths, diagonals=None):
    qd, qo = hip.pack(queries); rd, ro = hip.pack(refs)
    m, n = np.diff(qo).astype(np.float64), np.diff(ro).astype(np.float64)
    e_ms, e_info, e_rows, e_cig = timed(ctx.ends_plan(qd, qo, rd, ro, mat, go, ge, mode=mode, want_cigar=cigar, **GAP2))
    for w in widths:
        b_ms, b_info, b_rows, b_cig = timed(ctx.band_plan(qd, qo, rd, ro, mat, go, ge, w, mode=mode, diagonals=diagonals, want_cigar=cigar, **GAP2))
        cells = float(np.sum(m * (b_rows['band_hi'] - b_rows['band_lo'] + 1)))
        certified = same_rows(b_rows, b_cig, e_rows, e_cig, cigar, mode)
        print(json.dumps({'shape': name, 'pairs': len(queries), 'mode': mode, 'cigar': cigar, 'w': w, 'gap2': GAP2 or None,
                          'band_ms': round(b_ms, 3), 'band_cells': cells, 'band_gcups': round(cells / b_ms / 1e6, 2), 'band_shares': b_info['shares'],
                          'band_workspace': b_info['workspace_bytes'], 'class_pairs': b_info['class_pairs'],
                          'full_ms': round(e_ms, 3), 'full_cells': float(np.sum(m * n)), 'full_gcups': round(float(np.sum(m * n)) / e_ms / 1e6, 2),
                          'full_shares': e_info['shares'], 'full_workspace': e_info['workspace_bytes'],
                          'full_over_band': round(e_ms / b_ms, 2), 'certified': certified,
                          'equal_scores': int(np.sum(b_rows['score'] == e_rows['score']))}), flush=True)


def copies(rng, count, length):
    refs = [rng.integers(0, 4, length).astype(np.int8) for _ in range(count)]
    return [synth.mutate(r, rng, sub=0.04, ins=0.03, dele=0.03) for r in refs], refs


def flanks(rng, count=5000, length=1000, related=600):
    """seed-right flanks: the query is a 10 % mutated copy of the reference's first `related` letters, then unrelated letters"""
    refs = [rng.integers(0, 4, length).astype(np.int8) for _ in range(count)]
    queries = [np.concatenate([synth.mutate(r[:related], rng, sub=0.04, ins=0.03, dele=0.03), rng.integers(0, 4, length).astype(np.int8)])[:length]
               for r in refs]
    return queries, refs


def main():
    ctx = hip.default_context()
    rng = np.random.Generator(np.random.PCG64(20262))
    if 'a' in SHAPES or 'b' in SHAPES:
        queries, refs = copies(rng, N, 1000)
        if 'a' in SHAPES:
            shape(ctx, 'a: DNA 1 kb against 10 % mutated copies, global, score only', queries, refs, hip.score_matrix(*DNA[:2]), DNA[2], DNA[3], 'global', False, (32, 64, 128))
        if 'b' in SHAPES:
            shape(ctx, 'b: the same with CIGARs', queries, refs, hip.score_matrix(*DNA[:2]), DNA[2], DNA[3], 'global', True, (32, 64, 128))
    if 'c' in SHAPES:
        n = N + N // 4
        refs = [rng.integers(0, 4, 2000).astype(np.int8) for _ in range(n)]
        queries, diags = [], []
        for r in refs:
            at = int(rng.integers(0, 1950))
            q = synth.mutate(r[at:at + 50], rng, sub=0.04, ins=0.03, dele=0.03)
            queries.append(np.concatenate([q, rng.integers(0, 4, 50).astype(np.int8)])[:50])
            diags.append(at)
        shape(ctx, 'c: 50-nt junction in 2-kb reads, semiglobal, 10/4/8/2, hinted', queries, refs, hip.score_matrix(10, 4), 8, 2, 'semiglobal', False, (16,),
              diagonals=diags)
    if 'd' in SHAPES:
        queries, refs = copies(rng, max(1, N // 100), 20000)
        shape(ctx, 'd: DNA 20 kb x 20 kb with CIGARs', queries, refs, hip.score_matrix(*DNA[:2]), DNA[2], DNA[3], 'global', True, (128,))
    if 'e' in SHAPES or 'f' in SHAPES:
        queries, refs = flanks(np.random.Generator(np.random.PCG64(20263)))
        if 'e' in SHAPES:
            shape(ctx, 'e: 1-kb seed-right flanks, related for 600 letters, score only', queries, refs, hip.score_matrix(*DNA[:2]), DNA[2], DNA[3], MODE, False, (64,))
        if 'f' in SHAPES:
            shape(ctx, 'f: the same with CIGARs', queries, refs, hip.score_matrix(*DNA[:2]), DNA[2], DNA[3], MODE, True, (64,))


if __name__ == '__main__':
    main()
