"""K1g and K1gb under two-piece gap costs (csrc/ssw_ends.hip: `run`; csrc/ssw_band.hip: `run_band`, in the second half of this file) in
Python, for any geometry: the schemes of the kernels, not the definition (that is tests/twopiece_check.py).  K1g's geometry, modes
and end cells are those of tools/ends_model.py; costs = (go1, ge1, go2, ge2).  Per row step and lane:

    F_p[k] = max(Hprev[k] - go_p, F_pprev[k] - ge_p)               p = 1, 2, lane-private
    T[k]   = max(diag[k] + s, F_1[k], F_2[k])                      H without E
    V_p    = max over k of T[k] - go_p + (c + 1) ge_p              c = lane * cpl + k; one scan per piece, each in its own frame
    u_p    = exclusive prefix maximum of V_p over the lanes, lane 0 seeded with E_p of column 0 of the chunk
    e_p    = u_p - (lane * cpl) ge_p;  along the lane  E_p[k] = e_p,  H[k] = max(T[k], E_1[k], E_2[k]),  e_p = max(e_p - ge_p, T[k] - go_p)

The scan of piece p sees T - go_p and E_p - ge_p, never the other piece's E through H: the definition's cross term.  That the
term changes nothing the walk reads, under 0 <= ge2 <= ge1 <= go1 <= go2, is what tests/test_twopiece_host.py holds this model to
against the definition.  A chunk hands H, E_1 and E_2 of its last column on.  With `store` a cell leaves one byte: bits 0..2 H's
source (0 diagonal, 1 E_1, 2 E_2, 3 F_1, 4 F_2), bits 3..6 "opened here" of E_1, E_2, F_1, F_2.

`fault` plants one wrong line (the tests show that each is caught):
    'open2_go1'    piece 2 opened at go1              'handover_e2'  E_2 dropped from the chunk hand-over (E_1 handed in its place)
    'bit_e2'       E_2's "opened" bit read from E_1   'e2_first'     E_2 preferred over E_1 on a tie
    'boundary1'    the boundary gap costed by piece 1 alone"""
MODES = ('global', 'semiglobal', 'overlap', 'prefix', 'extend')
ANCHORED = ('global', 'prefix', 'extend')
FAULTS = ('open2_go1', 'handover_e2', 'bit_e2', 'e2_first', 'boundary1')


def _i32(v):
    assert -(1 << 31) <= v < (1 << 31), v
    return v


def run(q, r, mat, costs, mode, cpl=8, lanes=64, store=True, fault=None):
    """-> the result dict of tests/ends_check.py (begins and cigar None without `store`)"""
    go1, ge1, go2, ge2 = costs
    assert mode in MODES and 0 <= ge2 <= ge1 <= go1 <= go2 and fault in (None,) + FAULTS
    go = (go1, go1 if fault == 'open2_go1' else go2)
    ge = (ge1, ge2)
    m, n = len(q), len(r)
    assert m > 0 and n > 0, 'a pair with an empty side never reaches the kernel'

    def gap(k):
        a = go1 + (k - 1) * ge1
        return a if fault == 'boundary1' else min(a, go2 + (k - 1) * ge2)

    def row0(j):
        return -gap(j) if (mode in ANCHORED and j > 0) else 0

    def col0(i):
        return 0 if (mode == 'overlap' or i == 0) else -gap(i)
    C = cpl * lanes
    nchunks = (n + C - 1) // C
    hand = [None, None]
    row_best, row_j = col0(m), 0
    col_best, col_i = 0, 0
    corner = None
    ext = [(0, 0, 0)] * lanes
    cells = {}
    for c in range(nchunks):
        c0 = c * C
        cols = min(C, n - c0)
        last = c == nchunks - 1
        Hp = [[row0(c0 + 1 + l * cpl + k) for k in range(cpl)] for l in range(lanes)]
        Fp = [[[h - go[p] for h in Hp[l]] for l in range(lanes)] for p in (0, 1)]
        hleft = [Hp[l - 1][cpl - 1] if l else row0(c0) for l in range(lanes)]
        out = []
        ln, kn = (n - 1 - c0) // cpl, (n - 1 - c0) % cpl
        chunk_best = [None] * lanes
        for i in range(1, m + 1):
            if c == 0:
                hin = col0(i)
                E0 = [hin - go[p] for p in (0, 1)]
            else:
                hin, e_in = hand[(c - 1) & 1][i - 1]
                E0 = [max(e_in[p] - ge[p], hin - go[p]) for p in (0, 1)]
            T = [[0] * cpl for _ in range(lanes)]
            D = [[0] * cpl for _ in range(lanes)]
            F = [[[0] * cpl for _ in range(lanes)] for p in (0, 1)]
            V = [[0] * lanes, [0] * lanes]
            for l in range(lanes):
                v = [None, None]
                for k in range(cpl):
                    col = l * cpl + k
                    j = c0 + 1 + col
                    s = int(mat[r[j - 1]][q[i - 1]]) if j <= n else 0
                    for p in (0, 1):
                        F[p][l][k] = max(Hp[l][k] - go[p], Fp[p][l][k] - ge[p])
                    D[l][k] = (Hp[l][k - 1] if k else hleft[l]) + s
                    T[l][k] = max(D[l][k], F[0][l][k], F[1][l][k])
                    for p in (0, 1):
                        x = T[l][k] - go[p] + (col + 1) * ge[p]
                        v[p] = x if v[p] is None or x > v[p] else v[p]
                for p in (0, 1):
                    V[p][l] = max(v[p], E0[p]) if l == 0 else v[p]
            incl = [[], []]
            for p in (0, 1):
                run_ = None
                for l in range(lanes):
                    run_ = V[p][l] if run_ is None or V[p][l] > run_ else run_
                    incl[p].append(run_)
            H = [[0] * cpl for _ in range(lanes)]
            E = [[[0] * cpl for _ in range(lanes)] for p in (0, 1)]
            for l in range(lanes):
                e = [(incl[p][l - 1] if l else E0[p]) - l * cpl * ge[p] for p in (0, 1)]
                for k in range(cpl):
                    if c0 + 1 + l * cpl + k <= n:
                        _i32(e[0] + (l * cpl + k) * ge[0]); _i32(e[1] + (l * cpl + k) * ge[1]); _i32(T[l][k])
                    E[0][l][k], E[1][l][k] = e
                    H[l][k] = max(T[l][k], e[0], e[1])
                    e = [max(e[p] - ge[p], T[l][k] - go[p]) for p in (0, 1)]
            new_left = [H[l - 1][cpl - 1] if l else hin for l in range(lanes)]
            if store:
                for l in range((cols + cpl - 1) // cpl):
                    for k in range(cpl):
                        left = H[l][k - 1] if k else new_left[l]
                        h = H[l][k]
                        order = [D[l][k], E[0][l][k], E[1][l][k], F[0][l][k], F[1][l][k]]
                        src = order.index(h)
                        if fault == 'e2_first' and h != D[l][k] and h == E[1][l][k]:
                            src = 2
                        b = src
                        b |= 8 if E[0][l][k] == left - go[0] else 0
                        b |= 16 if E[0 if fault == 'bit_e2' else 1][l][k] == left - go[0 if fault == 'bit_e2' else 1] else 0
                        b |= 32 if F[0][l][k] == Hp[l][k] - go[0] else 0
                        b |= 64 if F[1][l][k] == Hp[l][k] - go[1] else 0
                        cells[(i, c0 + 1 + l * cpl + k)] = b
            if not last:
                e_out = (E[0][lanes - 1][cpl - 1], E[0 if fault == 'handover_e2' else 1][lanes - 1][cpl - 1])
                out.append((H[lanes - 1][cpl - 1], e_out))
            if mode == 'extend':
                for l in range(lanes):
                    for k in range(cpl):
                        if k < cols - l * cpl and (chunk_best[l] is None or H[l][k] > chunk_best[l][0]):
                            chunk_best[l] = (H[l][k], i, k)
            if i == m and mode in ('semiglobal', 'overlap', 'prefix'):
                for col in range(cols):
                    h = H[col // cpl][col % cpl]
                    if h > row_best:
                        row_best, row_j = h, c0 + 1 + col
            if last:
                hn = H[ln][kn]
                if i == m:
                    corner = hn
                elif mode == 'overlap' and hn > col_best:
                    col_best, col_i = hn, i
            Hp, Fp, hleft = H, F, new_left
        hand[c & 1] = out
        if mode == 'extend':
            for l in range(lanes):
                if chunk_best[l] is not None:
                    cv, ci, ck = chunk_best[l]
                    if cv > ext[l][0] or (cv == ext[l][0] and ci < ext[l][1]):
                        ext[l] = (cv, ci, c0 + 1 + l * cpl + ck)
    if mode == 'global':
        score, end = corner, (m, n)
    elif mode == 'extend':
        best = ext[0]
        for v2, i2, j2 in ext[1:]:
            if v2 > best[0] or (v2 == best[0] and (i2, j2) < (best[1], best[2])):
                best = (v2, i2, j2)
        score, end = best[0], (best[1], best[2])
    elif mode in ('semiglobal', 'prefix') or row_best >= col_best:
        score, end = row_best, (m, row_j)
    else:
        score, end = col_best, (col_i, n)
    res = {'score': score, 'ref_begin': None, 'ref_end': end[1] - 1, 'query_begin': None, 'query_end': end[0] - 1, 'cigar': None}
    if not store:
        return res
    i0, j0, ops = walk(cells, mode, end)
    res.update(ref_begin=j0, query_begin=i0, cigar=ops)
    return res


def walk(cells, mode, end):
    """one lane walks the stored bytes back (pr_walk<EN_TWO_PIECE> of csrc/ssw_pairs.h); at most i + j + 2 steps"""
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
                elif mode == 'semiglobal' and j == 0:
                    emit('I', i); i = 0
                break
        b = cells[(i, j)]
        if state == 0:
            state = b & 7                    # a gap state takes its first letter from this same cell
            if state == 0:
                emit('M'); i -= 1; j -= 1
                continue
        if state in (1, 2):
            emit('D'); j -= 1
        else:
            emit('I'); i -= 1
        if b & (4 << state):
            state = 0
    else:
        raise AssertionError('the walk did not end')
    return i, j, [(o, k) for o, k in reversed(ops)]


# ---- the band (csrc/ssw_band.hip) -------------------------------------------------------------------------------------------------
# K1gb's scheme (tools/band_model.py: the frame b = d - lo, F from position b + 1 of the row before, minus infinity as the int32
# NEG = -2^30, the sliding letters) with two pieces.  Per row step and lane:
#     F_p[k] = max(Hprev[k+1] - go_p, F_pprev[k+1] - ge_p)            T[k] = max(Hprev[k] + s, F_1[k], F_2[k])
#     X_p[k] = T[k] - go_p + (b + 1) ge_p where the position is a cell, else minus infinity;   V_p = max over k of X_p[k]
#     u_p    = exclusive prefix maximum of V_p over the lanes, seeded with minus infinity
#     E_p[k] = u_p - b ge_p,  H[k] = max(T[k], E_1[k], E_2[k]) where the position is a cell, else minus infinity,  u_p = max(u_p, X_p[k])
# Unlike K1g's two-piece kernel it keeps the u-form of the scan along the lane, and E, F and the "opened here" comparisons meet
# minus infinity: `run_band` checks value by value that every score stays inside (-2^29, 2^29) and everything derived from NEG
# inside [-2^30 - 2^29, -2^30 + 2^29) under the admission bound over all four costs (`band_admitted`).
# `fault`: 'open2_go1', 'bit_e2', 'e2_first', 'boundary1' as in `run`, and
#     'f2_own'    F_2 taken from position b instead of b + 1      'e2_seed'  E_2's scan seeded with a score instead of minus infinity
#     'exact1'    `exact` computed with piece 1 alone
NEG = -(1 << 30)
MAX_WIDTH = 512
BAND_MODES = ('global', 'semiglobal', 'prefix', 'extend')
BAND_FAULTS = ('open2_go1', 'bit_e2', 'e2_first', 'boundary1', 'f2_own', 'e2_seed', 'exact1')


def band_admitted(m, n, smax):
    """the range bound of clh_band_plan_create_gap2; smax is the greatest of |s|, go1, ge1, go2, ge2"""
    return (m + n + 2 * MAX_WIDTH) * max(smax, 1) < (1 << 29)


def band_exact(mode, m, n, lo, hi, score, splus, costs):
    """the host's certificate (clh_api.hip, bd_exact) with g, the cost of one run under the cheaper piece"""
    go1, ge1, go2, ge2 = costs

    def g(k):
        return min(go1 + (k - 1) * ge1, go2 + (k - 1) * ge2)
    if lo <= -m and hi >= n:
        return 1
    ok = True
    if mode in ('prefix', 'extend'):
        if hi + 1 <= n:
            ok = ok and score > splus * min(m, n - hi - 1) - g(hi + 1)
        if lo - 1 >= -m:
            ok = ok and score > splus * min(n, m + lo - 1) - g(1 - lo)
        return int(ok)
    if mode != 'global':
        return 0
    if hi + 1 <= n:
        ok = ok and score > splus * max(0, n - hi - 1) - g(hi + 1) - g(hi + 1 - (n - m))
    if lo - 1 >= -m:
        ok = ok and score > splus * max(0, m + lo - 1) - g(1 - lo) - g(n - m - lo + 1)
    return int(ok)


def _score(v):
    assert -(1 << 29) < v < (1 << 29), v
    return v


def _any(v):
    assert -(1 << 29) < v < (1 << 29) or -(1 << 30) - (1 << 29) <= v < -(1 << 30) + (1 << 29), v
    return v


def run_band(q, r, mat, costs, mode, lo, hi, cpl=8, lanes=64, store=True, fault=None):
    """-> the result dict of tests/twopiece_check.py's banded forms (begins and cigar None without `store`)"""
    go1, ge1, go2, ge2 = costs
    assert mode in BAND_MODES and 0 <= ge2 <= ge1 <= go1 <= go2 and fault in (None,) + BAND_FAULTS
    go = (go1, go1 if fault == 'open2_go1' else go2)
    ge = (ge1, ge2)
    m, n = len(q), len(r)
    assert m > 0 and n > 0, 'a pair with an empty side never reaches the kernel'
    W = cpl * lanes
    B = hi - lo + 1
    assert 1 <= B <= W and -m <= lo and hi <= n

    def gap(k):
        a = go1 + (k - 1) * ge1
        return a if fault == 'boundary1' else min(a, go2 + (k - 1) * ge2)

    def letter(j):
        return int(r[j - 1]) if 1 <= j <= n else 0
    jr = [lo + p + 1 if p < B else 1 << 30 for p in range(W)]
    rc = [letter(lo + p + 1) for p in range(W)]
    Hp, Fp = [], [[NEG] * W, [NEG] * W]
    for p in range(W):
        j0 = lo + p
        cell = p < B and 0 <= j0 <= n
        Hp.append((-gap(j0) if (mode in ANCHORED and j0 > 0) else 0) if cell else NEG)
    cells = {}
    H = Hp
    ext = [(0, 0, 0)] * lanes
    for i in range(1, m + 1):
        ok = [0 <= jr[p] <= n for p in range(W)]
        F = [[0] * W, [0] * W]
        D, T = [0] * W, [0] * W
        X = [[0] * W, [0] * W]
        for p in range(W):
            hu = Hp[p + 1] if p + 1 < W else NEG
            for t in (0, 1):
                fu = Fp[t][p + 1] if p + 1 < W else NEG
                if fault == 'f2_own' and t == 1:
                    F[t][p] = _any(max(Hp[p] - go[t], Fp[t][p] - ge[t]))
                else:
                    F[t][p] = _any(max(hu - go[t], fu - ge[t]))
            D[p] = _any(Hp[p] + int(mat[rc[p]][q[i - 1]]))
            T[p] = max(D[p], F[0][p], F[1][p])
            for t in (0, 1):
                X[t][p] = _score(_score(T[p]) - go[t] + (p + 1) * ge[t]) if ok[p] else NEG
        incl = [[], []]
        for t in (0, 1):
            best = NEG
            for l in range(lanes):
                best = max(best, max(X[t][l * cpl:(l + 1) * cpl]))
                incl[t].append(best)
        H = [0] * W
        E = [[0] * W, [0] * W]
        for l in range(lanes):
            u = [incl[t][l - 1] if l else (0 if (fault == 'e2_seed' and t == 1) else NEG) for t in (0, 1)]
            for k in range(cpl):
                p = l * cpl + k
                for t in (0, 1):
                    E[t][p] = _any(u[t] - p * ge[t])
                H[p] = _score(max(T[p], E[0][p], E[1][p])) if ok[p] else NEG
                u = [max(u[t], X[t][p]) for t in (0, 1)]
        if store:
            for p in range(B):
                left = H[p - 1] if p else NEG
                hu = Hp[p + 1] if p + 1 < W else NEG
                order = [D[p], E[0][p], E[1][p], F[0][p], F[1][p]]
                src = order.index(H[p]) if H[p] in order else 4          # a position that is no cell: never read
                if fault == 'e2_first' and H[p] != D[p] and H[p] == E[1][p]:
                    src = 2
                t2 = 0 if fault == 'bit_e2' else 1
                b = src | (8 if E[0][p] == left - go[0] else 0) | (16 if E[t2][p] == left - go[t2] else 0)
                b |= (32 if F[0][p] == hu - go[0] else 0) | (64 if F[1][p] == hu - go[1] else 0)
                cells[(i, i + lo + p)] = b
        if mode == 'extend':
            for p in range(W):
                if H[p] > ext[p // cpl][0]:
                    ext[p // cpl] = (H[p], i, jr[p])
        if i == m:
            last_ok = ok
            last_j = list(jr)
        Hp, Fp = H, F
        rc = rc[1:] + [letter(lo + W + i)]
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
    res = {'score': score, 'ref_begin': None, 'ref_end': end[1] - 1, 'query_begin': None, 'query_end': end[0] - 1, 'cigar': None, 'band': (lo, hi),
           'exact': band_exact(mode, m, n, lo, hi, score, splus, (go1, ge1, go1, ge1) if fault == 'exact1' else costs)}
    if not store:
        return res
    for (ci, cj) in cells:
        assert lo <= cj - ci <= hi
    i0, j0, ops = walk(cells, mode, end)             # a cell outside the band is a KeyError: the walk left the band
    res.update(ref_begin=j0, query_begin=i0, cigar=ops)
    return res
