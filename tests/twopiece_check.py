"""The definition of pair alignment under two-piece affine gap costs as ssw_wrap.align_pairs_ends / align_pairs_band (gap_open2=,
gap_extend2=) and clh_ends_plan_create_gap2 / clh_band_plan_create_gap2 state it (not a test module): the full dynamic programme in
Python integers for the five modes of tests/ends_check.py and tests/anchored_check.py, over the full matrix and, but for overlap,
over a band of diagonals (the band definition of tests/band_check.py), its end cell, and the walk back.

Costs are the tuple (go1, ge1, go2, ge2); a gap of k letters costs min(go1 + (k - 1) ge1, go2 + (k - 1) ge2).  In cells:

    E_p[i][j] = max(H[i][j-1] - go_p, E_p[i][j-1] - ge_p)      p = 1, 2      consumes a reference letter   (CIGAR D)
    F_p[i][j] = max(H[i-1][j] - go_p, F_p[i-1][j] - ge_p)      p = 1, 2      consumes a query letter       (CIGAR I)
    H[i][j]   = max(H[i-1][j-1] + s(q[i-1], r[j-1]), E_1, E_2, F_1, F_2),   H[0][0] = 0

Modes, boundaries, end cells and their ties, coordinates and CIGARs are those of the one-piece checkers; a boundary gap of j
letters costs the minimum over the pieces and each E_p / F_p of the boundary is its own piece's gap.  The walk prefers, in state
H, the diagonal, then E_1, E_2, F_1, F_2; in state E_p it emits D, moves left, and returns to H as soon as E_p[i][j] ==
H[i][j-1] - go_p (F_p likewise with I).  Both pieces emit the same op.  Admitted costs: 0 <= ge2 <= ge1 <= go1 <= go2
(`violated`): piece 1 for short gaps, piece 2 for long ones; under them a maximal run of D or I is never cheaper when split over
both pieces, which tests/test_twopiece_host.py checks against the enumeration of every alignment.

`plain` is the recurrence cell by cell; `align` builds each row with numpy for the larger GPU cases (E_p from H itself, in the
frame E_p[j] + j ge_p: the closed form of the recurrence, nothing assumed about the other piece).  `check_cigar` costs every
maximal run by the minimum, with no knowledge of tie rules, and demands the reported score."""
import numpy as np

import anchored_check as ac
import band_check as bc
import ends_check as ec

MODES = ec.MODES + ac.MODES
NEG = ec.NEG

rng_for = ec.rng_for
dna_matrix = ec.dna_matrix
encode = ec.encode
random_seq = ec.random_seq
mutate = ec.mutate
cigar_text = ec.cigar_text
parse_cigar = ec.parse_cigar
as_tuple = ec.as_tuple


def violated(costs):
    """the first inequality of 0 <= ge2 <= ge1 <= go1 <= go2 that the costs break -> a string, or None"""
    go1, ge1, go2, ge2 = costs
    if ge2 < 0:
        return '0 <= gap_extend2'
    if ge2 > ge1:
        return 'gap_extend2 <= gap_extend'
    if ge1 > go1:
        return 'gap_extend <= gap_open'
    if go1 > go2:
        return 'gap_open <= gap_open2'
    return None


def gap(k, costs):
    go1, ge1, go2, ge2 = costs
    return min(go1 + (k - 1) * ge1, go2 + (k - 1) * ge2)


def _anchored(mode):
    return mode in ('global', 'prefix', 'extend')


def _boundary(mode, m, n, costs):
    row0 = [0] + [-gap(j, costs) if _anchored(mode) else 0 for j in range(1, n + 1)]
    col0 = [0] + [0 if mode == 'overlap' else -gap(i, costs) for i in range(1, m + 1)]
    return row0, col0


def _end_cell(mode, m, n, H):
    """H(i, j) -> (i, j) of the end cell, by the rules of the one-piece checkers"""
    if mode in ec.MODES:
        return ec._end_cell(mode, m, n, [H(m, j) for j in range(n + 1)], [H(i, n) for i in range(m + 1)])
    return ac._end_cell(mode, m, n, [(i, j, H(i, j)) for i in range(m + 1) for j in range(n + 1)])[:2]


def _walk(mode, end, src, opened):
    """src(i, j): 0 diagonal, 1 E_1, 2 E_2, 3 F_1, 4 F_2, the first that equals H; opened(i, j, p): state p leaves its gap at (i, j)"""
    i, j = end
    ops = []

    def emit(op, k=1):
        if k <= 0:
            return
        if ops and ops[-1][0] == op:
            ops[-1][1] += k
        else:
            ops.append([op, k])
    state = 0
    while True:
        if state == 0:
            if _anchored(mode):
                if i == 0 or j == 0:
                    emit('D', j); emit('I', i)       # one of them is zero: the remaining letters are one gap
                    i = j = 0
                    break
            else:
                if i == 0:
                    break
                if j == 0:
                    if mode == 'semiglobal':
                        emit('I', i); i = 0
                    break
            state = src(i, j)
            if state == 0:
                emit('M'); i -= 1; j -= 1
        elif state in (1, 2):
            emit('D')
            if opened(i, j, state):
                state = 0
            j -= 1
        else:
            emit('I')
            if opened(i, j, state):
                state = 0
            i -= 1
    return i, j, [(o, k) for o, k in reversed(ops)]


def plain(q, r, mat, costs, mode):
    """the recurrence, one cell after the other, in Python integers"""
    assert mode in MODES and violated(costs) is None
    go = (None, costs[0], costs[2]); ge = (None, costs[1], costs[3])
    m, n = len(q), len(r)
    H = [[NEG] * (n + 1) for _ in range(m + 1)]
    D = [[NEG] * (n + 1) for _ in range(m + 1)]
    E = [None] + [[[NEG] * (n + 1) for _ in range(m + 1)] for _ in (1, 2)]
    F = [None] + [[[NEG] * (n + 1) for _ in range(m + 1)] for _ in (1, 2)]
    row0, col0 = _boundary(mode, m, n, costs)
    for j in range(n + 1):
        H[0][j] = row0[j]
        if _anchored(mode) and j:
            for p in (1, 2):
                E[p][0][j] = -(go[p] + (j - 1) * ge[p])
    for i in range(1, m + 1):
        H[i][0] = col0[i]
        if mode != 'overlap':
            for p in (1, 2):
                F[p][i][0] = -(go[p] + (i - 1) * ge[p])
    for i in range(1, m + 1):
        for j in range(1, n + 1):
            for p in (1, 2):
                E[p][i][j] = max(H[i][j - 1] - go[p], E[p][i][j - 1] - ge[p])
                F[p][i][j] = max(H[i - 1][j] - go[p], F[p][i - 1][j] - ge[p])
            D[i][j] = H[i - 1][j - 1] + int(mat[r[j - 1]][q[i - 1]])
            H[i][j] = max(D[i][j], E[1][i][j], E[2][i][j], F[1][i][j], F[2][i][j])
    end = _end_cell(mode, m, n, lambda i, j: H[i][j])

    def src(i, j):
        return [D[i][j], E[1][i][j], E[2][i][j], F[1][i][j], F[2][i][j]].index(H[i][j])

    def opened(i, j, s):
        if s <= 2:
            return E[s][i][j] == H[i][j - 1] - go[s]
        return F[s - 2][i][j] == H[i - 1][j] - go[s - 2]
    i0, j0, ops = _walk(mode, end, src, opened)
    return ec._result(H[end[0]][end[1]], end, (i0, j0), ops)


def align(q, r, mat, costs, mode, path=True):
    """the same programme row by row in numpy int64; path=False: score and end cell only (begins and cigar None)"""
    assert mode in MODES and violated(costs) is None
    go = (None, costs[0], costs[2]); ge = (None, costs[1], costs[3])
    q = np.asarray(q, dtype=np.int64); r = np.asarray(r, dtype=np.int64)
    mat = np.asarray(mat, dtype=np.int64)
    m, n = len(q), len(r)
    row0, col0 = _boundary(mode, m, n, costs)
    ar = [None] + [np.arange(n + 1, dtype=np.int64) * ge[p] for p in (1, 2)]
    Hp = np.array(row0, dtype=np.int64)
    Fp = [None, np.full(n + 1, NEG, dtype=np.int64), np.full(n + 1, NEG, dtype=np.int64)]
    flags = np.zeros((m + 1, n + 1), dtype=np.uint8) if path else None      # bits 0..2 the source, 3..6 opened here: E_1, E_2, F_1, F_2
    last_col = [int(Hp[n])]
    best = (0, 0, 0)                                                        # extend: (i, j, H), the first of the greatest in row order
    for i in range(1, m + 1):
        F = [None] + [np.maximum(Hp - go[p], Fp[p] - ge[p]) for p in (1, 2)]
        T = np.empty(n + 1, dtype=np.int64)
        T[0] = col0[i]
        d = Hp[:-1] + mat[r, q[i - 1]] if n else np.zeros(0, dtype=np.int64)
        T[1:] = np.maximum(d, np.maximum(F[1][1:], F[2][1:]))
        # H first, from the scans over T = max(diagonal, F_1, F_2); then each E_p from H itself, which is the recurrence's closed form,
        # and H again from those: the two must agree (the other piece's E never lifts an E_p above H)
        E = [None, np.full(n + 1, NEG, dtype=np.int64), np.full(n + 1, NEG, dtype=np.int64)]
        H = T.copy()
        if n:
            for p in (1, 2):
                H[1:] = np.maximum(H[1:], np.maximum.accumulate(T[:-1] - go[p] + ar[p][1:]) - ar[p][1:])
            for p in (1, 2):
                E[p][1:] = np.maximum.accumulate(H[:-1] - go[p] + ar[p][1:]) - ar[p][1:]
            assert (np.maximum(T, np.maximum(E[1], E[2])) == H).all(), i
        if path and n:
            h = H[1:]
            s = np.where(h == d, 0, np.where(h == E[1][1:], 1, np.where(h == E[2][1:], 2, np.where(h == F[1][1:], 3, 4)))).astype(np.uint8)
            assert ((s < 4) | (h == F[2][1:])).all()
            for p in (1, 2):
                s |= (E[p][1:] == H[:-1] - go[p]).astype(np.uint8) << (2 + p)
                s |= (F[p][1:] == Hp[1:] - go[p]).astype(np.uint8) << (4 + p)
            flags[i, 1:] = s
        Hp = H
        for p in (1, 2):
            Fp[p] = F[p]
            Fp[p][0] = NEG if mode == 'overlap' else -(go[p] + (i - 1) * ge[p])
        last_col.append(int(Hp[n]))
        jb = int(np.argmax(H))
        if int(H[jb]) > best[2]:
            best = (i, jb, int(H[jb]))
    if mode in ec.MODES:
        end = ec._end_cell(mode, m, n, [int(x) for x in Hp], last_col)
        score = int(Hp[end[1]]) if end[0] == m else last_col[end[0]]
    else:
        if mode == 'prefix':
            jb = int(np.argmax(Hp))
            best = (m, jb, int(Hp[jb]))
        end, score = best[:2], best[2]
    if not path:
        return {'score': score, 'ref_begin': None, 'ref_end': end[1] - 1, 'query_begin': None, 'query_end': end[0] - 1, 'cigar': None}
    i0, j0, ops = _walk(mode, end, lambda i, j: int(flags[i, j]) & 7, lambda i, j, s: (int(flags[i, j]) >> (2 + s)) & 1)
    return ec._result(score, end, (i0, j0), ops)


# ---- the band -----------------------------------------------------------------------------------------------------------------
BAND_MODES = ('global', 'semiglobal', 'prefix', 'extend')
_FIN = NEG // 2          # anything below is minus infinity (a sum that started from NEG)


def band_of(mode, m, n, w, diag=None):
    """the clipped band [lo, hi] of a pair: band_check's for the end-anchored modes, anchored_check's for the start-anchored ones"""
    return bc.band_of(m, n, w, diag) if mode in bc.MODES else ac.band_of(m, n, w, diag)


def refusal(mode, m, n, lo, hi):
    return bc.refusal(mode, m, n, lo, hi) if mode in bc.MODES else ac.refusal(mode, m, n, lo, hi)


def exact_flag(mode, m, n, lo, hi, score, mat, costs):
    """1: it is proved that the unbanded programme returns the same row and CIGAR; 0: not proved.  The certificates of band_check and
    anchored_check with g(L) = gap(L, costs) for the cost of the run that reaches diagonal hi + 1 (lo - 1) and, in the global mode,
    of the run that comes back to diagonal n - m.  All the proofs ask of g is that it does not decrease and that g(a) + g(b) >=
    g(a + b): several runs that add up to L letters cost at least one run of L.  The comparison is strict."""
    if lo <= -m and hi >= n:
        return 1
    sp = max(0, int(np.max(mat))) if np.size(mat) else 0
    ok = True
    if mode in ac.MODES:
        if hi + 1 <= n:
            ok = ok and score > sp * min(m, n - hi - 1) - gap(hi + 1, costs)
        if lo - 1 >= -m:
            ok = ok and score > sp * min(n, m + lo - 1) - gap(1 - lo, costs)
        return int(ok)
    if mode != 'global':
        return 0
    if hi + 1 <= n:
        ok = ok and score > sp * max(0, n - hi - 1) - gap(hi + 1, costs) - gap(hi + 1 - (n - m), costs)
    if lo - 1 >= -m:
        ok = ok and score > sp * max(0, m + lo - 1) - gap(1 - lo, costs) - gap(n - m - lo + 1, costs)
    return int(ok)


def _fin(v):
    return v if v > _FIN else NEG


def _band_end(mode, m, n, cells):
    """cells: (i, j, H) of the band's cells in ascending (i, j) -> (i, j) of the end cell"""
    if mode == 'global':
        return m, n
    if mode == 'semiglobal':
        mode = 'prefix'                                # the greatest H[m][j] over the band's cells of row m, smallest j
    return ac._end_cell(mode, m, n, cells)[:2]


def _band_result(score, end, begin, ops, mode, m, n, lo, hi, mat, costs):
    res = ec._result(score, end, begin, ops)
    res['band'] = (lo, hi)
    res['exact'] = exact_flag(mode, m, n, lo, hi, int(score), mat, costs)
    return res


def plain_band(q, r, mat, costs, mode, lo, hi):
    """the banded recurrence, one cell after the other, in Python integers; [lo, hi] is the clipped band.  Cells outside are minus
    infinity; row 0 and column 0 are produced by the recurrences from (0, 0) (semiglobal: H[0][j] = 0 on the band's cells of row 0)"""
    assert mode in BAND_MODES and violated(costs) is None
    go = (None, costs[0], costs[2]); ge = (None, costs[1], costs[3])
    m, n = len(q), len(r)
    assert -m <= lo <= hi <= n and refusal(mode, m, n, lo, hi) is None

    def inb(i, j):
        return 0 <= i <= m and 0 <= j <= n and lo <= j - i <= hi
    H = [[NEG] * (n + 1) for _ in range(m + 1)]
    D = [[NEG] * (n + 1) for _ in range(m + 1)]
    E = [None] + [[[NEG] * (n + 1) for _ in range(m + 1)] for _ in (1, 2)]
    F = [None] + [[[NEG] * (n + 1) for _ in range(m + 1)] for _ in (1, 2)]
    cells = []
    for i in range(m + 1):
        for j in range(n + 1):
            if not inb(i, j):
                continue
            if i == 0 and (j == 0 or mode == 'semiglobal'):
                H[i][j] = 0
            else:
                for p in (1, 2):
                    if inb(i, j - 1):
                        E[p][i][j] = _fin(max(H[i][j - 1] - go[p], E[p][i][j - 1] - ge[p]))
                    if inb(i - 1, j):
                        F[p][i][j] = _fin(max(H[i - 1][j] - go[p], F[p][i - 1][j] - ge[p]))
                if i and j:
                    D[i][j] = _fin(H[i - 1][j - 1] + int(mat[r[j - 1]][q[i - 1]]))
                H[i][j] = max(D[i][j], E[1][i][j], E[2][i][j], F[1][i][j], F[2][i][j])
            assert H[i][j] > _FIN, (i, j)            # every cell of an admitted band is reached from a start cell
            cells.append((i, j, H[i][j]))
    end = _band_end(mode, m, n, cells)

    def src(i, j):
        return [D[i][j], E[1][i][j], E[2][i][j], F[1][i][j], F[2][i][j]].index(H[i][j])

    def opened(i, j, s):
        if s <= 2:
            return E[s][i][j] == H[i][j - 1] - go[s]
        return F[s - 2][i][j] == H[i - 1][j] - go[s - 2]
    i0, j0, ops = _walk(mode, end, src, opened)
    return _band_result(H[end[0]][end[1]], end, (i0, j0), ops, mode, m, n, lo, hi, mat, costs)


def align_band(q, r, mat, costs, mode, lo, hi, path=True):
    """the banded programme row by row in numpy int64, in the band's frame: position b of row i is the cell (i, i + lo + b)"""
    assert mode in BAND_MODES and violated(costs) is None
    go = (None, costs[0], costs[2]); ge = (None, costs[1], costs[3])
    q = np.asarray(q, dtype=np.int64); r = np.asarray(r, dtype=np.int64)
    mat = np.asarray(mat, dtype=np.int64)
    m, n = len(q), len(r)
    assert -m <= lo <= hi <= n and refusal(mode, m, n, lo, hi) is None
    B = hi - lo + 1
    pos = np.arange(B, dtype=np.int64)
    ar = [None, pos * ge[1], pos * ge[2]]
    letters = np.zeros(2 * m + n + 2, dtype=np.int64)      # letters[x] is the reference letter of column x - m (0 outside the reference)
    letters[m:m + n] = r
    j0 = lo + pos
    ok0 = (j0 >= 0) & (j0 <= n)
    if mode == 'semiglobal':
        Hp = np.where(ok0, 0, NEG)
    else:
        jj = np.maximum(j0, 1)
        Hp = np.where(ok0, np.where(j0 > 0, -np.minimum(go[1] + (jj - 1) * ge[1], go[2] + (jj - 1) * ge[2]), 0), NEG)
    Fp = [None, np.full(B, NEG, dtype=np.int64), np.full(B, NEG, dtype=np.int64)]
    flags = np.zeros((m + 1, B), dtype=np.uint8) if path else None
    best = (0, 0, 0)
    for i in range(1, m + 1):
        j = i + lo + pos
        ok = (j >= 0) & (j <= n)
        Hup = np.append(Hp[1:], NEG)
        F = [None]
        for p in (1, 2):
            f = np.maximum(Hup - go[p], np.append(Fp[p][1:], NEG) - ge[p])
            f[f < _FIN] = NEG
            F.append(f)
        d = Hp + mat[letters[j - 1 + m], q[i - 1]]
        d[(d < _FIN) | (j < 1)] = NEG
        T = np.where(ok, np.maximum(d, np.maximum(F[1], F[2])), NEG)
        H = T.copy()
        E = [None, np.full(B, NEG, dtype=np.int64), np.full(B, NEG, dtype=np.int64)]
        if B > 1:
            for p in (1, 2):
                H[1:] = np.maximum(H[1:], np.maximum.accumulate(T[:-1] - go[p] + ar[p][1:]) - ar[p][1:])
            H = np.where(ok & (H > _FIN), H, NEG)
            for p in (1, 2):                                  # E_p from H itself: the recurrence's closed form
                E[p][1:] = np.maximum.accumulate(H[:-1] - go[p] + ar[p][1:]) - ar[p][1:]
                E[p][E[p] < _FIN] = NEG
            assert (np.where(ok, np.maximum(T, np.maximum(E[1], E[2])), NEG) == H).all(), i
        if path:
            left = np.insert(H[:-1], 0, NEG)
            s = np.where(H == d, 0, np.where(H == E[1], 1, np.where(H == E[2], 2, np.where(H == F[1], 3, 4)))).astype(np.uint8)
            for p in (1, 2):
                s |= ((E[p] == left - go[p]) & (left > _FIN)).astype(np.uint8) << (2 + p)
                s |= ((F[p] == Hup - go[p]) & (Hup > _FIN)).astype(np.uint8) << (4 + p)
            flags[i] = np.where(ok, s, 0)
        Hp = H
        for p in (1, 2):
            Fp[p] = np.where(ok, F[p], NEG)
        b = int(np.argmax(H))
        if int(H[b]) > best[2]:
            best = (i, int(j[b]), int(H[b]))
    if mode == 'global':
        best = (m, n, int(Hp[n - m - lo]))
    elif mode != 'extend':
        b = int(np.argmax(Hp)) if m else int(np.argmax(np.where(ok0, Hp, NEG)))
        best = (m, m + lo + b, int(Hp[b]))
    end, score = best[:2], best[2]
    if not path:
        res = {'score': score, 'ref_begin': None, 'ref_end': end[1] - 1, 'query_begin': None, 'query_end': end[0] - 1, 'cigar': None}
        res['band'] = (lo, hi)
        res['exact'] = exact_flag(mode, m, n, lo, hi, score, mat, costs)
        return res
    i0, jb, ops = _walk(mode, end, lambda i, jj: int(flags[i, jj - i - lo]) & 7, lambda i, jj, s: (int(flags[i, jj - i - lo]) >> (2 + s)) & 1)
    return _band_result(score, end, (i0, jb), ops, mode, m, n, lo, hi, mat, costs)


def as_tuple_band(res):
    return as_tuple(res) + (tuple(res['band']), int(res['exact']))


def rescore(cigar, q, r, ref_begin, query_begin, mat, costs):
    """what a CIGAR costs with every maximal run of I or D at the cheaper piece -> (score, reference letters, query letters); the
    columns and the spans are ends_check.rescore's, with free gaps"""
    runs = []
    for op, k in cigar:
        if runs and runs[-1][0] == op:
            runs[-1][1] += k
        else:
            runs.append([op, k])
    score, nr, nq = ec.rescore(cigar, q, r, ref_begin, query_begin, mat, 0, 0)
    return score - sum(gap(k, costs) for op, k in runs if op != 'M'), nr, nq


def check_cigar(res, q, r, mat, costs, mode):
    """the CIGAR of a result rescores to its score and spans exactly its coordinates; the spans are what the mode allows"""
    m, n = len(q), len(r)
    score, nr, nq = rescore(res['cigar'], q, r, res['ref_begin'], res['query_begin'], mat, costs)
    assert score == res['score'], (score, res)
    assert res['ref_begin'] + nr - 1 == res['ref_end'] and res['query_begin'] + nq - 1 == res['query_end'], (nr, nq, res)
    assert 0 <= res['ref_begin'] <= res['ref_end'] + 1 <= n and 0 <= res['query_begin'] <= res['query_end'] + 1 <= m, res
    ops = [o for o, _ in res['cigar']]
    assert all(a != b for a, b in zip(ops, ops[1:])), res['cigar']
    if _anchored(mode):
        assert (res['ref_begin'], res['query_begin']) == (0, 0), res
    if mode == 'global':
        assert (res['ref_end'], res['query_end']) == (n - 1, m - 1), res
    elif mode in ('semiglobal', 'prefix'):
        assert (res['query_begin'], res['query_end']) == (0, m - 1), res
    elif mode == 'overlap':
        assert res['ref_begin'] == 0 or res['query_begin'] == 0
        assert res['ref_end'] == n - 1 or res['query_end'] == m - 1
    else:
        assert res['score'] >= 0 and (res['score'] > 0 or (res['ref_end'], res['query_end'], res['cigar']) == (-1, -1, [])), res
    if 'band' in res:
        lo, hi = res['band']
        assert all(lo <= j - i <= hi for i, j in bc.cells_of(res)), res


def stitch(left, right, ref_pos, query_pos, seed_len=0, seed_score=0):
    """what extend_anchors returns for one pair from its two `extend` halves (anchored_check.stitch)"""
    return ac.stitch(left, right, ref_pos, query_pos, seed_len, seed_score)


def expected_anchor(rs, qs, anchor, seed_len, scoring, band=None):
    """the checker's stitched answer for one pair; scoring = (match, mismatch, go1, ge1, go2, ge2) -> (tuple of as_tuple, exact of
    both halves)"""
    mat = dna_matrix(scoring[0], scoring[1])
    costs = tuple(scoring[2:])
    rp, qp = anchor
    halves = []
    for rh, qh in ((rs[:rp][::-1], qs[:qp][::-1]), (rs[rp + seed_len:], qs[qp + seed_len:])):
        q, r = encode(qh), encode(rh)
        if band is None:
            halves.append(align(q, r, mat, costs, 'extend'))
        else:
            halves.append(align_band(q, r, mat, costs, 'extend', *band_of('extend', len(q), len(r), band)))
    seed = sum(int(mat[a][b]) for a, b in zip(encode(rs[rp:rp + seed_len]), encode(qs[qp:qp + seed_len])))
    return stitch(halves[0], halves[1], rp, qp, seed_len, seed), all(h.get('exact', 1) for h in halves)
