"""K1g (csrc/ssw_ends.hip) in Python, for any geometry: the scheme of the kernel, not the definition (that is tests/ends_check.py).

One wave takes one pair.  Its `lanes` lanes own `cpl` consecutive reference columns each, so a chunk is lanes * cpl columns; a
longer reference is walked chunk after chunk, every chunk over all query rows, and a chunk hands the H and E of its last column
on, one pair of values per row.  Per row step and lane:

    F[k]  = max(Hprev[k] - go, Fprev[k] - ge)                       lane-private
    T[k]  = max(diag[k] + s, F[k])                                  H without E
    V     = max over k of T[k] - go + (p + 1) ge                    p = lane * cpl + k, the column inside the chunk
    U     = exclusive prefix maximum of V over the lanes, lane 0 seeded with E of column 0 of the chunk
    E[k]  = u - p ge,  H[k] = max(T[k], E[k]),  u = max(u, T[k] - go + (p + 1) ge)      the scan in the frame E[p] + p ge

which is E[j] = max(E[j-1] - ge, H[j-1] - go) exactly when go >= ge.  No cell holds minus infinity: F of row 0 and E of column
0 enter as H - go, which gives the same first F and E.  With `store`, each cell leaves 4 bits -- H's source (0 diagonal, 1 E, 2
F), "E opened here", "F opened here" -- a word of cpl nibbles per lane and row, and one lane walks them back.  Values are
checked to stay inside int32.

The start-anchored modes (tests/anchored_check.py) have global's boundary and walk.  `prefix` ends at the last row's running
maximum, seeded with H[m][0].  `extend` ends at the greatest H of all cells, smallest i, then smallest j, (0, 0) with 0 included:
every lane keeps the best (value, i, k) of its own cells of a chunk under a bare > (rows ascend, its columns ascend within a row),
joins it at the end of the chunk to the best it carries by the key -- a later chunk's columns are larger, its rows may be smaller
-- and the lanes are reduced once, after the last chunk."""
MODES = ('global', 'semiglobal', 'overlap', 'prefix', 'extend')
ANCHORED = ('global', 'prefix', 'extend')          # row 0 is one gap from (0, 0), the walk stops at (0, 0)


def _i32(v):
    assert -(1 << 31) <= v < (1 << 31), v
    return v


def _row0(mode, j, go, ge):
    return -(go + (j - 1) * ge) if (mode in ANCHORED and j > 0) else 0


def _col0(mode, i, go, ge):
    return 0 if (mode == 'overlap' or i == 0) else -(go + (i - 1) * ge)


def run(q, r, mat, go, ge, mode, cpl=8, lanes=64, store=True, extreme=None):
    """-> the result dict of tests/ends_check.py (begins and cigar None without `store`); `extreme`, a list, receives the largest
    magnitude among the values checked to stay inside int32"""
    assert mode in MODES and go >= ge >= 0
    m, n = len(q), len(r)
    assert m > 0 and n > 0, 'a pair with an empty side never reaches the kernel'
    C = cpl * lanes
    nchunks = (n + C - 1) // C
    hand = [None, None]
    row_best, row_j = _col0(mode, m, go, ge), 0           # running maximum of the last row, smallest j
    col_best, col_i = 0, 0                                # of the last column (overlap): H[0][n] = 0
    corner = None
    ext = [(0, 0, 0)] * lanes                             # extend: (value, i, j) of the best cell a lane has seen, seeded with (0, 0)
    words = {}
    peak = 0
    for c in range(nchunks):
        c0 = c * C
        cols = min(C, n - c0)
        last = c == nchunks - 1
        Hp = [[_row0(mode, c0 + 1 + l * cpl + k, go, ge) for k in range(cpl)] for l in range(lanes)]
        Fp = [[h - go for h in Hp[l]] for l in range(lanes)]
        hleft = [Hp[l - 1][cpl - 1] if l else _row0(mode, c0, go, ge) for l in range(lanes)]     # H[i-1][first column - 1]
        out = []
        ln, kn = (n - 1 - c0) // cpl, (n - 1 - c0) % cpl
        chunk_best = [None] * lanes                       # extend: (value, i, k) of this chunk's best per lane
        for i in range(1, m + 1):
            if c == 0:
                hin = _col0(mode, i, go, ge)
                ein = hin - go
            else:
                hin, ein = hand[(c - 1) & 1][i - 1]
            E0 = max(ein - ge, hin - go)
            T = [[0] * cpl for _ in range(lanes)]
            F = [[0] * cpl for _ in range(lanes)]
            D = [[0] * cpl for _ in range(lanes)]
            V = [0] * lanes
            for l in range(lanes):
                v = None
                for k in range(cpl):
                    p = l * cpl + k
                    j = c0 + 1 + p
                    s = int(mat[r[j - 1]][q[i - 1]]) if j <= n else 0
                    diag = Hp[l][k - 1] if k else hleft[l]
                    F[l][k] = max(Hp[l][k] - go, Fp[l][k] - ge)
                    D[l][k] = diag + s
                    T[l][k] = max(D[l][k], F[l][k])
                    x = T[l][k] - go + (p + 1) * ge
                    v = x if v is None or x > v else v
                V[l] = max(v, E0) if l == 0 else v
            incl, run_ = [], None
            for l in range(lanes):
                run_ = V[l] if run_ is None or V[l] > run_ else run_
                incl.append(run_)
            H = [[0] * cpl for _ in range(lanes)]
            E = [[0] * cpl for _ in range(lanes)]
            for l in range(lanes):
                u = incl[l - 1] if l else E0
                for k in range(cpl):
                    p = l * cpl + k
                    if c0 + 1 + p <= n:
                        _i32(u); _i32(T[l][k])
                        peak = max(peak, abs(u), abs(T[l][k]))
                    E[l][k] = u - p * ge
                    H[l][k] = max(T[l][k], E[l][k])
                    x = T[l][k] - go + (p + 1) * ge
                    u = x if x > u else u
            new_left = [H[l - 1][cpl - 1] if l else hin for l in range(lanes)]          # H[i][first column - 1]
            if store:
                for l in range((cols + cpl - 1) // cpl):
                    w = 0
                    for k in range(cpl):
                        left = H[l][k - 1] if k else new_left[l]
                        src = 0 if H[l][k] == D[l][k] else (1 if H[l][k] == E[l][k] else 2)
                        nib = src | (4 if E[l][k] == left - go else 0) | (8 if F[l][k] == Hp[l][k] - go else 0)
                        w |= nib << (4 * k)
                    words[(c, i, l)] = w
            if not last:
                out.append((H[lanes - 1][cpl - 1], E[lanes - 1][cpl - 1]))
            if mode == 'extend':
                for l in range(lanes):
                    for k in range(cpl):
                        if k < cols - l * cpl and (chunk_best[l] is None or H[l][k] > chunk_best[l][0]):
                            chunk_best[l] = (H[l][k], i, k)
            if i == m and mode in ('semiglobal', 'overlap', 'prefix'):
                for p in range(cols):
                    h = H[p // cpl][p % cpl]
                    if h > row_best:
                        row_best, row_j = h, c0 + 1 + p
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
    if extreme is not None:
        extreme.append(peak)
    if mode == 'global':
        score, end = corner, (m, n)
    elif mode == 'extend':
        best = ext[0]
        for v2, i2, j2 in ext[1:]:                        # the butterfly's order of comparisons does not matter: the key is total
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
    i0, j0, ops = walk(words, mode, end, cpl, lanes)
    res.update(ref_begin=j0, query_begin=i0, cigar=ops)
    if mode in ('prefix', 'extend'):
        assert (i0, j0) == (0, 0)
    return res


def walk(words, mode, end, cpl, lanes):
    """one lane walks the stored nibbles back; at most i + j + 2 steps"""
    C = cpl * lanes
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
        p = (j - 1) % C
        nib = (words[((j - 1) // C, i, p // cpl)] >> (4 * (p % cpl))) & 15
        if state == 0:
            state = nib & 3                  # a gap state takes its first letter from this same cell
            if state == 0:
                emit('M'); i -= 1; j -= 1
                continue
        if state == 1:
            emit('D'); j -= 1
            if nib & 4:
                state = 0
        else:
            emit('I'); i -= 1
            if nib & 8:
                state = 0
    else:
        raise AssertionError('the walk did not end')
    return i, j, [(o, k) for o, k in reversed(ops)]
