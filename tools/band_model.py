"""K1gb (csrc/ssw_band.hip) in Python, for any geometry: the scheme of the kernel, not the definition (that is tests/band_check.py).

One wave takes one pair, in the frame of its band [lo, hi] of diagonals d = j - i.  Its `lanes` lanes own `cpl` consecutive band
positions b = d - lo each (the band must fit: hi - lo + 1 <= lanes * cpl), the loop runs over the query rows, and position b of row
i is the cell (i, i + lo + b).  The diagonal source is the position's own value of the row before, F's source is position b + 1
of the row before, E along the row is the max-plus prefix scan of K1g.  Per row step and lane:

    F[k]  = max(Hprev[k+1] - go, Fprev[k+1] - ge)                   position lanes * cpl, past the last lane, is minus infinity
    T[k]  = max(Hprev[k] + s, F[k])                                 H without E
    X[k]  = T[k] - go + (p + 1) ge where the position is a cell, else minus infinity;   V = max over k of X[k]
    u     = exclusive prefix maximum of V over the lanes, seeded with minus infinity
    E[k]  = u - p ge,  H[k] = max(T[k], E[k]) where the position is a cell, else minus infinity,  u = max(u, X[k])

A position is a cell of row i while b < B and 0 <= j <= n.  The cell of column 0 needs no rule of its own: the position held
minus infinity in the row before and nothing lies to its left, so H = F, the gap from (0, 0), while the band holds the cells above.
The reference letter of a position moves by one per row: the letters slide down the positions, one new letter enters at the top
position per row.  Minus infinity is NEG = -2^30, an ordinary int32 that is added to like any other: the admission bound
(`admitted`) keeps every score inside (-2^29, 2^29) and everything derived from NEG inside [-2^30 - 2^29, -2^30 + 2^29), which `run`
checks value by value.  With `store`, each cell leaves 4 bits -- H's source (0 diagonal, 1 E, 2 F), "E opened here", "F opened
here" -- and one lane walks them back in the band's frame: a diagonal step keeps b, a D step goes to b - 1, an I step to b + 1.

The start-anchored modes (tests/anchored_check.py) have global's row 0 and walk; their far end is free, so the default band is
[-w, w] (`band_of`).  `prefix` ends where semiglobal does.  `extend` ends at the greatest H over the band's cells, smallest i, then
smallest j: a lane keeps the best of its own cells under a bare >, seeded with (0, (0, 0)), which the cells of column 0 (<= 0)
and minus infinity never beat, and the lanes are reduced once by the key after the last row."""
MODES = ('global', 'semiglobal', 'prefix', 'extend')
ANCHORED = ('global', 'prefix', 'extend')          # row 0 is one gap from (0, 0), the walk stops at (0, 0)
NEG = -(1 << 30)
MAX_WIDTH = 512


def admitted(m, n, smax):
    """the range bound of clh_band_plan_create"""
    return (m + n + 2 * MAX_WIDTH) * max(smax, 1) < (1 << 29)


def band_of(mode, m, n, w, diag=None):
    """the clipped band clh_band_plan_create gives a pair"""
    if diag is not None:
        lo, hi = diag - w, diag + w
    elif mode in ('prefix', 'extend'):
        lo, hi = -w, w
    else:
        lo, hi = min(0, n - m) - w, max(0, n - m) + w
    return max(lo, -m), min(hi, n)


def exact_flag(mode, m, n, lo, hi, score, splus, go, ge):
    """the host's certificate (clh_api.hip, bd_exact)"""
    if lo <= -m and hi >= n:
        return 1
    if mode in ('prefix', 'extend'):
        free = True
        if hi + 1 <= n:
            free = free and score > splus * min(m, n - hi - 1) - go - hi * ge
        if lo - 1 >= -m:
            free = free and score > splus * min(n, m + lo - 1) - go - (-lo) * ge
        return int(free)
    if mode != 'global':
        return 0
    ok = True
    if hi + 1 <= n:
        ok = ok and score > splus * max(0, n - hi - 1) - 2 * go - (2 * (hi + 1) - (n - m) - 2) * ge
    if lo - 1 >= -m:
        ok = ok and score > splus * max(0, m + lo - 1) - 2 * go - (2 * (1 - lo) + (n - m) - 2) * ge
    return int(ok)


def _score(v):
    assert -(1 << 29) < v < (1 << 29), v
    return v


def _any(v):
    assert -(1 << 29) < v < (1 << 29) or -(1 << 30) - (1 << 29) <= v < -(1 << 30) + (1 << 29), v
    return v


def run(q, r, mat, go, ge, mode, lo, hi, cpl=8, lanes=64, store=True):
    """-> the result dict of tests/band_check.py (begins and cigar None without `store`)"""
    assert mode in MODES and go >= ge >= 0
    m, n = len(q), len(r)
    assert m > 0 and n > 0, 'a pair with an empty side never reaches the kernel'
    W = cpl * lanes
    B = hi - lo + 1
    assert 1 <= B <= W and -m <= lo and hi <= n

    def letter(j):                                   # the letter of column j, 0 outside the reference
        return int(r[j - 1]) if 1 <= j <= n else 0
    jr = [lo + p + 1 if p < B else 1 << 30 for p in range(W)]      # the position's column in the row at hand
    rc = [letter(lo + p + 1) for p in range(W)]
    Hp, Fp = [], [NEG] * W
    for p in range(W):
        j0 = lo + p
        cell = p < B and 0 <= j0 <= n
        Hp.append((-(go + (j0 - 1) * ge) if (mode in ANCHORED and j0 > 0) else 0) if cell else NEG)
    nib = {}
    H = Hp
    ext = [(0, 0, 0)] * lanes                        # extend: (value, i, j) of the best cell a lane has seen, seeded with (0, 0)
    for i in range(1, m + 1):
        ok = [0 <= jr[p] <= n for p in range(W)]
        F, D, T, X = [0] * W, [0] * W, [0] * W, [0] * W
        for p in range(W):
            hu = Hp[p + 1] if p + 1 < W else NEG
            fu = Fp[p + 1] if p + 1 < W else NEG
            F[p] = _any(max(hu - go, fu - ge))
            D[p] = _any(Hp[p] + int(mat[rc[p]][q[i - 1]]))
            T[p] = max(D[p], F[p])
            X[p] = _score(_score(T[p]) - go + (p + 1) * ge) if ok[p] else NEG
        V = [max(X[l * cpl:(l + 1) * cpl]) for l in range(lanes)]
        incl, best = [], NEG
        for l in range(lanes):
            best = max(best, V[l])
            incl.append(best)
        H, E = [0] * W, [0] * W
        for l in range(lanes):
            u = incl[l - 1] if l else NEG
            for k in range(cpl):
                p = l * cpl + k
                E[p] = _any(u - p * ge)
                H[p] = _score(max(T[p], E[p])) if ok[p] else NEG
                u = max(u, X[p])
        if store:
            for p in range(B):
                left = H[p - 1] if p else NEG
                hu = Hp[p + 1] if p + 1 < W else NEG
                src = 0 if H[p] == D[p] else (1 if H[p] == E[p] else 2)
                nib[(i, p)] = src | (4 if E[p] == left - go else 0) | (8 if F[p] == hu - go else 0)
        if mode == 'extend':
            for p in range(W):
                if H[p] > ext[p // cpl][0]:
                    ext[p // cpl] = (H[p], i, jr[p])
        if i == m:
            last_ok = ok
            last_j = list(jr)
        Hp, Fp = H, F
        rc = rc[1:] + [letter(lo + W + i)]           # the letters slide down; the top position's next column is i + 1 + lo + W - 1
        jr = [j + 1 for j in jr]
    if mode == 'global':
        score, end = H[n - m - lo], (m, n)
    elif mode == 'extend':
        best = ext[0]
        for v2, i2, j2 in ext[1:]:
            if v2 > best[0] or (v2 == best[0] and (i2, j2) < (best[1], best[2])):
                best = (v2, i2, j2)
        score, end = best[0], (best[1], best[2])
    else:
        score, end = None, None
        for p in range(W):
            if last_ok[p] and (score is None or H[p] > score):
                score, end = H[p], (m, last_j[p])
    splus = max(0, max(int(x) for row in mat for x in row))
    res = {'score': score, 'ref_begin': None, 'ref_end': end[1] - 1, 'query_begin': None, 'query_end': end[0] - 1, 'cigar': None,
           'band': (lo, hi), 'exact': exact_flag(mode, m, n, lo, hi, score, splus, go, ge)}
    if not store:
        return res
    i0, j0, ops = walk(nib, mode, end, lo, B)
    res.update(ref_begin=j0, query_begin=i0, cigar=ops)
    return res


def walk(nib, mode, end, lo, B):
    """one lane walks the stored nibbles back; at most i + j + 2 steps"""
    i, j = end
    ops, state = [], 0

    def emit(op, k=1):
        if k <= 0:
            return
        if ops and ops[-1][0] == op:
            ops[-1][1] += k
        else:
            ops.append([op, k])
    for _ in range(end[0] + end[1] + 2):
        if state == 0:
            if i == 0 or j == 0:
                if mode in ANCHORED:
                    emit('D', j); emit('I', i); i = j = 0
                elif j == 0:
                    emit('I', i); i = 0
                break
        b = j - i - lo
        assert 0 <= b < B, 'the walk left the band'
        x = nib[(i, b)]
        if state == 0:
            state = x & 3                    # a gap state takes its first letter from this same cell
            if state == 0:
                emit('M'); i -= 1; j -= 1
                continue
        if state == 1:
            emit('D'); j -= 1
            if x & 4:
                state = 0
        else:
            emit('I'); i -= 1
            if x & 8:
                state = 0
    else:
        raise AssertionError('the walk did not end')
    return i, j, [(o, k) for o, k in reversed(ops)]
