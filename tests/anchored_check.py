"""The definition of start-anchored affine-gap alignment of a pair (modes prefix, extend) as ssw_wrap.align_pairs_ends,
align_pairs_band, extend_anchors and clh_ends_* / clh_band_* state it (not a test module).

Cells, recurrences, go >= ge >= 0, the walk's tie rules, coordinates and CIGARs are those of tests/ends_check.py.  Both modes are
pinned at (0, 0): row 0 and column 0 are global's (one gap from (0, 0)), ref_begin = query_begin = 0, the walk is global's and
stops at (0, 0), and letters beyond the end cell are not part of the CIGAR.

    prefix  the whole query against a prefix of the reference: the end cell is the greatest H[m][j], 0 <= j <= n, smallest j
    extend  a prefix of the query against a prefix of the reference: the end cell is the greatest H[i][j] over all cells, (0, 0)
            with H = 0 included, smallest i, then smallest j; the score is >= 0, the empty result has ref_end = query_end = -1

Over a band [lo, hi] of diagonals d = j - i (tests/band_check.py) the far end is free, so without a hint the band is [-w, w], and
with a hint [diag - w, diag + w], both clipped to [-m, n]; it must hold diagonal 0, and for prefix a cell of row m (`refusal`).
Cells outside the band are minus infinity and the end cell is taken over the band's cells only.  `exact_flag` is this module's own
statement of the certificate that the unbanded programme returns the same row and CIGAR.

`plain` / `plain_band` are the recurrences cell by cell in Python integers; `align` / `align_band` build each row with numpy (the
band in its own frame, position b = d - lo) for the larger GPU cases.  Results are the dicts of ends_check (plus 'band' and
'exact' under a band).  `stitch` is what extend_anchors returns, from two `extend` results."""
import numpy as np

import band_check as bc
import ends_check as ec

MODES = ('prefix', 'extend')
NEG = ec.NEG
_FIN = NEG // 2

rng_for = ec.rng_for
dna_matrix = ec.dna_matrix
encode = ec.encode
rescore = ec.rescore
random_seq = ec.random_seq
mutate = ec.mutate
cigar_text = ec.cigar_text
parse_cigar = ec.parse_cigar
as_tuple = ec.as_tuple


def _gap(k, go, ge):
    return go + (k - 1) * ge


def _end_cell(mode, m, n, cells):
    """cells: (i, j, H) of the candidate cells in ascending (i, j); -> (i, j, H) of the end cell"""
    if mode == 'prefix':
        best = None
        for i, j, h in cells:
            if i == m and (best is None or h > best[2]):
                best = (i, j, h)
        return best
    best = (0, 0, 0)
    for i, j, h in cells:
        if h > best[2]:
            best = (i, j, h)
    return best


def plain(q, r, mat, go, ge, mode):
    """the recurrence over the full matrix, one cell after the other, in Python integers"""
    assert mode in MODES and go >= ge >= 0
    m, n = len(q), len(r)
    H = [[NEG] * (n + 1) for _ in range(m + 1)]
    E = [[NEG] * (n + 1) for _ in range(m + 1)]
    F = [[NEG] * (n + 1) for _ in range(m + 1)]
    H[0][0] = 0
    for j in range(1, n + 1):
        H[0][j] = E[0][j] = -_gap(j, go, ge)
    for i in range(1, m + 1):
        H[i][0] = F[i][0] = -_gap(i, go, ge)
    for i in range(1, m + 1):
        for j in range(1, n + 1):
            E[i][j] = max(H[i][j - 1] - go, E[i][j - 1] - ge)
            F[i][j] = max(H[i - 1][j] - go, F[i - 1][j] - ge)
            H[i][j] = max(H[i - 1][j - 1] + int(mat[r[j - 1]][q[i - 1]]), E[i][j], F[i][j])
    ei, ej, score = _end_cell(mode, m, n, [(i, j, H[i][j]) for i in range(m + 1) for j in range(n + 1)])
    i0, j0, ops = ec._walk('global', (ei, ej),
                           lambda i, j: H[i][j] == H[i - 1][j - 1] + int(mat[r[j - 1]][q[i - 1]]),
                           lambda i, j: H[i][j] == E[i][j], lambda i, j: H[i][j] == F[i][j],
                           lambda i, j: E[i][j] == H[i][j - 1] - go, lambda i, j: F[i][j] == H[i - 1][j] - go)
    assert (i0, j0) == (0, 0)
    return ec._result(score, (ei, ej), (0, 0), ops)


def align(q, r, mat, go, ge, mode, path=True):
    """the same programme row by row in numpy int64"""
    assert mode in MODES and go >= ge >= 0
    q = np.asarray(q, dtype=np.int64); r = np.asarray(r, dtype=np.int64)
    mat = np.asarray(mat, dtype=np.int64)
    m, n = len(q), len(r)
    ar = np.arange(n + 1, dtype=np.int64) * ge
    Hp = np.array([0] + [-_gap(j, go, ge) for j in range(1, n + 1)], dtype=np.int64)
    Fp = np.full(n + 1, NEG, dtype=np.int64)
    flags = np.zeros((m + 1, n + 1), dtype=np.uint8) if path else None
    best = (0, 0, 0)
    for i in range(1, m + 1):
        c0 = -_gap(i, go, ge)
        F = np.maximum(Hp - go, Fp - ge)
        T = np.empty(n + 1, dtype=np.int64)
        T[0] = c0
        d = Hp[:-1] + mat[r, q[i - 1]] if n else np.zeros(0, dtype=np.int64)
        T[1:] = np.maximum(d, F[1:])
        E = np.full(n + 1, NEG, dtype=np.int64)
        if n:
            E[1:] = np.maximum.accumulate(T[:-1] - go + ar[1:]) - ar[1:]
        H = np.maximum(T, E)
        H[0] = c0
        if path and n:
            f = (H[1:] == d).astype(np.uint8) | ((H[1:] == E[1:]).astype(np.uint8) << 1) | ((H[1:] == F[1:]).astype(np.uint8) << 2)
            f |= ((E[1:] == H[:-1] - go).astype(np.uint8) << 3) | ((F[1:] == Hp[1:] - go).astype(np.uint8) << 4)
            flags[i, 1:] = f
        Hp, Fp = H, F
        Fp[0] = c0
        jb = int(np.argmax(H))                       # the first of equal maxima: the smallest j
        if int(H[jb]) > best[2]:
            best = (i, jb, int(H[jb]))
    if mode == 'prefix':
        jb = int(np.argmax(Hp))
        best = (m, jb, int(Hp[jb]))
    ei, ej, score = best
    if not path:
        return {'score': score, 'ref_begin': None, 'ref_end': ej - 1, 'query_begin': None, 'query_end': ei - 1, 'cigar': None}
    i0, j0, ops = ec._walk('global', (ei, ej), lambda i, j: flags[i, j] & 1, lambda i, j: flags[i, j] & 2, lambda i, j: flags[i, j] & 4,
                           lambda i, j: flags[i, j] & 8, lambda i, j: flags[i, j] & 16)
    return ec._result(score, (ei, ej), (i0, j0), ops)


# ---- the band ---------------------------------------------------------------------------------------------------------------
def band_unclipped(w, diag=None):
    return (-w, w) if diag is None else (diag - w, diag + w)


def band_of(m, n, w, diag=None):
    """the clipped band [lo, hi] of a pair: the far end is free, so n - m plays no part"""
    lo, hi = band_unclipped(w, diag)
    return max(lo, -m), min(hi, n)


def refusal(mode, m, n, lo, hi):
    """why a band (before or after clipping) admits no alignment -> a string, or None"""
    if lo > 0 or hi < 0:
        return 'misses (0, 0)'
    if mode == 'prefix' and lo > n - m:
        return 'no end cell'
    return None


def exact_flag(mode, m, n, lo, hi, score, mat, go, ge):
    """1: it is proved that the unbanded programme returns the same row and CIGAR; 0: not proved.  An alignment from (0, 0) that
    leaves the band has a cell on diagonal hi + 1 or lo - 1 and need not come back.  Reaching hi + 1 takes at least hi + 1 D letters
    in at least one run, which leaves at most min(m, n - hi - 1) M columns, each worth at most s+ = max(0, greatest matrix entry);
    mirrored below.  STRICTLY above every defined bound, every alignment that reaches the optimum at any end cell lies in the
    band: the best cells, their tie and the walk's comparisons are the same."""
    assert mode in MODES
    if lo <= -m and hi >= n:
        return 1
    sp = max(0, int(np.max(mat))) if np.size(mat) else 0
    ok = True
    if hi + 1 <= n:
        ok = ok and score > sp * min(m, n - hi - 1) - go - hi * ge
    if lo - 1 >= -m:
        ok = ok and score > sp * min(n, m + lo - 1) - go - (-lo) * ge
    return int(ok)


def _fin(v):
    return v if v > _FIN else NEG


def _band_result(score, end, ops, mode, m, n, lo, hi, mat, go, ge):
    res = ec._result(score, end, (0, 0), ops)
    res['band'] = (lo, hi)
    res['exact'] = exact_flag(mode, m, n, lo, hi, int(score), mat, go, ge)
    return res


def plain_band(q, r, mat, go, ge, mode, lo, hi):
    """the banded recurrence, one cell after the other, in Python integers; [lo, hi] is the clipped band"""
    assert mode in MODES and go >= ge >= 0
    m, n = len(q), len(r)
    assert -m <= lo <= hi <= n and refusal(mode, m, n, lo, hi) is None

    def inb(i, j):
        return 0 <= i <= m and 0 <= j <= n and lo <= j - i <= hi
    H = [[NEG] * (n + 1) for _ in range(m + 1)]
    E = [[NEG] * (n + 1) for _ in range(m + 1)]
    F = [[NEG] * (n + 1) for _ in range(m + 1)]
    D = [[NEG] * (n + 1) for _ in range(m + 1)]
    cells = []
    for i in range(m + 1):
        for j in range(n + 1):
            if not inb(i, j):
                continue
            if i == 0 and j == 0:
                H[i][j] = 0
            else:
                if inb(i, j - 1):
                    E[i][j] = _fin(max(H[i][j - 1] - go, E[i][j - 1] - ge))
                if inb(i - 1, j):
                    F[i][j] = _fin(max(H[i - 1][j] - go, F[i - 1][j] - ge))
                if i and j:
                    D[i][j] = _fin(H[i - 1][j - 1] + int(mat[r[j - 1]][q[i - 1]]))
                H[i][j] = max(D[i][j], E[i][j], F[i][j])
            assert H[i][j] > _FIN, (i, j)            # every cell of an admitted band is reached from (0, 0)
            cells.append((i, j, H[i][j]))
    ei, ej, score = _end_cell(mode, m, n, cells)
    i0, j0, ops = ec._walk('global', (ei, ej),
                           lambda i, j: H[i][j] == D[i][j],
                           lambda i, j: H[i][j] == E[i][j], lambda i, j: H[i][j] == F[i][j],
                           lambda i, j: E[i][j] == H[i][j - 1] - go, lambda i, j: F[i][j] == H[i - 1][j] - go)
    assert (i0, j0) == (0, 0)
    return _band_result(score, (ei, ej), ops, mode, m, n, lo, hi, mat, go, ge)


def align_band(q, r, mat, go, ge, mode, lo, hi, path=True):
    """the banded programme row by row in numpy int64, in the band's frame: position b of row i is the cell (i, i + lo + b)"""
    assert mode in MODES and go >= ge >= 0
    q = np.asarray(q, dtype=np.int64); r = np.asarray(r, dtype=np.int64)
    mat = np.asarray(mat, dtype=np.int64)
    m, n = len(q), len(r)
    assert -m <= lo <= hi <= n and refusal(mode, m, n, lo, hi) is None
    B = hi - lo + 1
    pos = np.arange(B, dtype=np.int64)
    ar = pos * ge
    letters = np.zeros(2 * m + n + 2, dtype=np.int64)
    letters[m:m + n] = r
    j0 = lo + pos
    ok0 = (j0 >= 0) & (j0 <= n)
    Hp = np.where(ok0, np.where(j0 > 0, -(go + (j0 - 1) * ge), 0), NEG)
    Fp = np.full(B, NEG, dtype=np.int64)
    flags = np.zeros((m + 1, B), dtype=np.uint8) if path else None
    best = (0, 0, 0)
    for i in range(1, m + 1):
        j = i + lo + pos
        ok = (j >= 0) & (j <= n)
        Hup = np.append(Hp[1:], NEG); Fup = np.append(Fp[1:], NEG)
        F = np.maximum(Hup - go, Fup - ge)
        F[F < _FIN] = NEG
        d = Hp + mat[letters[j - 1 + m], q[i - 1]]
        d[(d < _FIN) | (j < 1)] = NEG
        T = np.where(ok, np.maximum(d, F), NEG)
        E = np.full(B, NEG, dtype=np.int64)
        if B > 1:
            E[1:] = np.maximum.accumulate(T[:-1] - go + ar[1:]) - ar[1:]
        E[E < _FIN] = NEG
        H = np.where(ok, np.maximum(T, E), NEG)
        if path:
            left = np.insert(H[:-1], 0, NEG)
            f = (H == d).astype(np.uint8) | ((H == E).astype(np.uint8) << 1) | ((H == F).astype(np.uint8) << 2)
            f |= ((E == left - go).astype(np.uint8) << 3) | ((F == Hup - go).astype(np.uint8) << 4)
            flags[i] = np.where(ok, f, 0)
        Hp, Fp = H, np.where(ok, F, NEG)
        b = int(np.argmax(H))
        if int(H[b]) > best[2]:
            best = (i, int(j[b]), int(H[b]))
    if mode == 'prefix':
        b = int(np.argmax(Hp)) if m else int(np.argmax(np.where(ok0, Hp, NEG)))
        best = (m, m + lo + b, int(Hp[b]))
    ei, ej, score = best
    if not path:
        res = {'score': score, 'ref_begin': None, 'ref_end': ej - 1, 'query_begin': None, 'query_end': ei - 1, 'cigar': None}
        res['band'] = (lo, hi)
        res['exact'] = exact_flag(mode, m, n, lo, hi, score, mat, go, ge)
        return res

    def bit(x):
        return lambda i, jj: flags[i, jj - i - lo] & x
    i0, jb, ops = ec._walk('global', (ei, ej), bit(1), bit(2), bit(4), bit(8), bit(16))
    assert (i0, jb) == (0, 0)
    return _band_result(score, (ei, ej), ops, mode, m, n, lo, hi, mat, go, ge)


def check_cigar(res, q, r, mat, go, ge, mode):
    """the CIGAR rescores to the score (a rescore that knows no tie rule) and spans exactly the coordinates; the spans are what the
    mode allows; under a band every cell lies inside it"""
    m, n = len(q), len(r)
    score, nr, nq = rescore(res['cigar'], q, r, 0, 0, mat, go, ge)
    assert score == res['score'], (score, res)
    assert res['ref_begin'] == 0 and res['query_begin'] == 0, res
    assert nr - 1 == res['ref_end'] and nq - 1 == res['query_end'], (nr, nq, res)
    assert nr <= n and nq <= m, res
    ops = [o for o, _ in res['cigar']]
    assert all(a != b for a, b in zip(ops, ops[1:])), res['cigar']
    if mode == 'prefix':
        assert res['query_end'] == m - 1, res
    else:
        assert res['score'] >= 0 and (res['score'] > 0 or (res['ref_end'], res['query_end'], res['cigar']) == (-1, -1, [])), res
    if 'band' in res:
        lo, hi = res['band']
        assert all(lo <= j - i <= hi for i, j in bc.cells_of(res)), res


def stitch(left, right, ref_pos, query_pos, seed_len=0, seed_score=0):
    """what extend_anchors returns for one pair, from the `extend` result of the reversed letters before the anchor (left) and of
    the letters after it and its seed (right): the tuple of ends_check.as_tuple, in the coordinates of the whole sequences"""
    ops = []
    for o, k in list(reversed(left['cigar'])) + ([('M', seed_len)] if seed_len else []) + list(right['cigar']):
        if ops and ops[-1][0] == o:
            ops[-1] = (o, ops[-1][1] + k)
        else:
            ops.append((o, k))
    return (left['score'] + seed_score + right['score'],
            ref_pos - (left['ref_end'] + 1), ref_pos + seed_len + right['ref_end'],
            query_pos - (left['query_end'] + 1), query_pos + seed_len + right['query_end'], cigar_text(ops))


def anchored_reads(rng, count, seed_len=20, lo=30, hi=120):
    """reads with a planted exact seed: (reference, query, (ref_pos, query_pos) of the seed's first letter); the flanks are 10 %
    mutated copies that turn unrelated some way out, of different lengths on either side"""
    out = []
    for t in range(count):
        seed = random_seq(rng, seed_len)
        sides = []
        for _ in range(2):
            core = random_seq(rng, rng.randint(0, hi - lo))
            sides.append((core + random_seq(rng, rng.randint(0, lo)), mutate(rng, core, 0.10) + random_seq(rng, rng.randint(0, lo))))
        (lr, lq), (rr, rq) = sides
        out.append((lr[::-1] + seed + rr, lq[::-1] + seed + rq, (len(lr), len(lq))))
    return out


def expected_anchor(rs, qs, anchor, seed_len, scoring, band=None):
    """the checker's stitched answer for one pair -> (tuple of ends_check.as_tuple, exact of both halves)"""
    ma, mi, go, ge = scoring
    mat = dna_matrix(ma, mi)
    rp, qp = anchor
    halves = []
    for r, q in ((rs[:rp][::-1], qs[:qp][::-1]), (rs[rp + seed_len:], qs[qp + seed_len:])):
        q, r = encode(q), encode(r)
        if band is None:
            halves.append(align(q, r, mat, go, ge, 'extend'))
        else:
            halves.append(align_band(q, r, mat, go, ge, 'extend', *band_of(len(q), len(r), band)))
    seed = sum(int(mat[a][b]) for a, b in zip(encode(rs[rp:rp + seed_len]), encode(qs[qp:qp + seed_len])))
    return stitch(halves[0], halves[1], rp, qp, seed_len, seed), all(h.get('exact', 1) for h in halves)


def text_of(want, m):
    """the cigar_string of a stitched answer: soft clips around the ops, as PyAlignRes writes them"""
    tail = m - want[4] - 1
    return ('%dS' % want[3] if want[3] > 0 else '') + want[5] + ('%dS' % tail if tail else '')
