"""The definition of banded end-anchored alignment of a pair (modes global, semiglobal) as ssw_wrap.align_pairs_band and
clh_band_* state it (not a test module).

The band of a pair of m query and n reference letters is a closed interval of diagonals [lo, hi], d = j - i (i query letters, j
reference letters consumed, as in tests/ends_check.py): with half-width w and no hint lo = min(0, n - m) - w, hi = max(0, n - m)
+ w; with a hint `diag`, lo = diag - w, hi = diag + w; both clipped to [-m, n] (`band_of`).  The programme is that of
ends_check with every cell outside the band at minus infinity in H, E and F, and row 0 and column 0 produced by the same
recurrences from (0, 0) rather than filled in:

    E[i][j] = max(H[i][j-1] - go, E[i][j-1] - ge)      if (i, j-1) is in the band, else -inf
    F[i][j] = max(H[i-1][j] - go, F[i-1][j] - ge)      if (i-1, j) is in the band, else -inf
    H[i][j] = max(H[i-1][j-1] + s(q[i-1], r[j-1]), E[i][j], F[i][j]),   H[0][0] = 0 where the band holds it
    semiglobal: H[0][j] = 0 on the band's cells of row 0 (E[0][j] = -inf)

so every score is the score of an alignment all of whose cells lie in the band.  The end cell is (m, n) (global) or the greatest
H[m][j] over the band's cells of row m, smallest j (semiglobal); the walk back is ends_check's, and a source outside the band
is no source.  `refusal` states which bands have no alignment at all.

`plain` is the recurrence cell by cell in Python integers; `align` builds each row with numpy in the band's own frame (position
b = d - lo), so a 3000 x 3000 pair under a band of 65 diagonals costs 3000 short rows.  `exact_flag` is the certificate that
the unbanded programme returns the same row and CIGAR.  Results are the dicts of ends_check plus 'band' = (lo, hi) and 'exact'."""
import numpy as np

import ends_check as ec

MODES = ('global', 'semiglobal')
NEG = ec.NEG
_FIN = NEG // 2          # anything below is minus infinity (a sum that started from NEG)

rng_for = ec.rng_for
dna_matrix = ec.dna_matrix
encode = ec.encode
random_seq = ec.random_seq
mutate = ec.mutate
cigar_text = ec.cigar_text
parse_cigar = ec.parse_cigar
rescore = ec.rescore


def band_of(m, n, w, diag=None):
    """the clipped band [lo, hi] of a pair"""
    if diag is None:
        lo, hi = min(0, n - m) - w, max(0, n - m) + w
    else:
        lo, hi = diag - w, diag + w
    return max(lo, -m), min(hi, n)


def refusal(mode, m, n, lo, hi):
    """why a band (before or after clipping) admits no alignment -> a string, or None"""
    if mode == 'global':
        if lo > min(0, n - m) or hi < max(0, n - m):
            return 'misses (0, 0) or (m, n)'
    elif hi < 0 or lo > n - m:
        return 'no start cell or no end cell'
    return None


def exact_flag(mode, m, n, lo, hi, score, mat, go, ge):
    """1: it is proved that the unbanded programme returns the same row and CIGAR; 0: not proved.  A global alignment that leaves
    the band reaches diagonal hi + 1 or lo - 1, and so has at least two gap runs and a bounded number of M columns: with s+ =
    max(0, greatest matrix entry) no such alignment scores above ub_top resp. ub_bot, and STRICTLY above both every optimal
    alignment, hence every comparison the walk makes on an optimal path, lies in the band."""
    if lo <= -m and hi >= n:
        return 1
    if mode != 'global':
        return 0
    sp = max(0, int(np.max(mat))) if np.size(mat) else 0
    ok = True
    if hi + 1 <= n:
        ok &= score > sp * max(0, n - hi - 1) - 2 * go - (2 * (hi + 1) - (n - m) - 2) * ge
    if lo - 1 >= -m:
        ok &= score > sp * max(0, m + lo - 1) - 2 * go - (2 * (1 - lo) + (n - m) - 2) * ge
    return int(ok)


def _fin(v):
    return v if v > _FIN else NEG


def _end_cell(mode, m, n, lo, hi, hrow):
    """hrow(j) = H[m][j]"""
    if mode == 'global':
        return m, n
    best, cell = None, None
    for j in range(max(0, m + lo), min(n, m + hi) + 1):
        if best is None or hrow(j) > best:
            best, cell = hrow(j), (m, j)
    return cell


def _result(score, end, begin, ops, mode, m, n, lo, hi, mat, go, ge):
    res = ec._result(score, end, begin, ops)
    res['band'] = (lo, hi)
    res['exact'] = exact_flag(mode, m, n, lo, hi, int(score), mat, go, ge)
    return res


def plain(q, r, mat, go, ge, mode, lo, hi):
    """the recurrence, one cell after the other, in Python integers; [lo, hi] is the clipped band"""
    assert mode in MODES and go >= ge >= 0
    m, n = len(q), len(r)
    assert -m <= lo <= hi <= n and refusal(mode, m, n, lo, hi) is None

    def inb(i, j):
        return 0 <= i <= m and 0 <= j <= n and lo <= j - i <= hi
    H = [[NEG] * (n + 1) for _ in range(m + 1)]
    E = [[NEG] * (n + 1) for _ in range(m + 1)]
    F = [[NEG] * (n + 1) for _ in range(m + 1)]
    D = [[NEG] * (n + 1) for _ in range(m + 1)]
    for i in range(m + 1):
        for j in range(n + 1):
            if not inb(i, j):
                continue
            if i == 0 and (j == 0 or mode == 'semiglobal'):
                H[i][j] = 0
                continue
            if inb(i, j - 1):
                E[i][j] = _fin(max(H[i][j - 1] - go, E[i][j - 1] - ge))
            if inb(i - 1, j):
                F[i][j] = _fin(max(H[i - 1][j] - go, F[i - 1][j] - ge))
            if i and j:
                D[i][j] = _fin(H[i - 1][j - 1] + int(mat[r[j - 1]][q[i - 1]]))
            H[i][j] = max(D[i][j], E[i][j], F[i][j])
            assert H[i][j] > _FIN, (i, j)            # every cell of an admitted band is reached
    end = _end_cell(mode, m, n, lo, hi, lambda j: H[m][j])
    i0, j0, ops = ec._walk(mode, end,
                           lambda i, j: H[i][j] == D[i][j],
                           lambda i, j: H[i][j] == E[i][j], lambda i, j: H[i][j] == F[i][j],
                           lambda i, j: E[i][j] == H[i][j - 1] - go, lambda i, j: F[i][j] == H[i - 1][j] - go)
    return _result(H[end[0]][end[1]], end, (i0, j0), ops, mode, m, n, lo, hi, mat, go, ge)


def align(q, r, mat, go, ge, mode, lo, hi, path=True):
    """the same programme row by row in numpy int64, in the band's frame: position b of row i is the cell (i, i + lo + b)"""
    assert mode in MODES and go >= ge >= 0
    q = np.asarray(q, dtype=np.int64); r = np.asarray(r, dtype=np.int64)
    mat = np.asarray(mat, dtype=np.int64)
    m, n = len(q), len(r)
    assert -m <= lo <= hi <= n and refusal(mode, m, n, lo, hi) is None
    B = hi - lo + 1
    pos = np.arange(B, dtype=np.int64)
    ar = pos * ge
    # letters[x] is the reference letter of column x - m (0 outside the reference), so that row i reads letters[i + lo + b - 1 + m]
    letters = np.zeros(2 * m + n + 2, dtype=np.int64)
    letters[m:m + n] = r
    j0 = lo + pos
    ok0 = (j0 >= 0) & (j0 <= n)
    if mode == 'global':
        Hp = np.where(ok0, np.where(j0 > 0, -(go + (j0 - 1) * ge), 0), NEG)
    else:
        Hp = np.where(ok0, 0, NEG)
    Fp = np.full(B, NEG, dtype=np.int64)
    flags = np.zeros((m + 1, B), dtype=np.uint8) if path else None
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
    end = _end_cell(mode, m, n, lo, hi, lambda jj: int(Hp[jj - m - lo]))
    score = int(Hp[end[1] - m - lo])
    if not path:
        res = {'score': score, 'ref_begin': None, 'ref_end': end[1] - 1, 'query_begin': None, 'query_end': end[0] - 1, 'cigar': None}
        res['band'] = (lo, hi)
        res['exact'] = exact_flag(mode, m, n, lo, hi, score, mat, go, ge)
        return res

    def bit(x):
        return lambda i, jj: flags[i, jj - i - lo] & x
    i0, jb, ops = ec._walk(mode, end, bit(1), bit(2), bit(4), bit(8), bit(16))
    return _result(score, end, (i0, jb), ops, mode, m, n, lo, hi, mat, go, ge)


def cells_of(res):
    """the cells (i, j) a result's alignment visits, both ends included"""
    i, j = res['query_begin'], res['ref_begin']
    out = [(i, j)]
    for op, k in res['cigar']:
        for _ in range(k):
            i += op in 'MI'; j += op in 'MD'
            out.append((i, j))
    return out


def check_cigar(res, q, r, mat, go, ge, mode):
    """ends_check.check_cigar (a rescore that knows no tie rule, spans, what the mode allows), and every cell inside the band"""
    ec.check_cigar(res, q, r, mat, go, ge, mode)
    lo, hi = res['band']
    assert all(lo <= j - i <= hi for i, j in cells_of(res)), res


def as_tuple(res):
    return ec.as_tuple(res) + (tuple(res['band']), int(res['exact']))
