"""K1g with intron gaps (csrc/ssw_ends.hip) in Python, for any geometry: the scheme of the kernel, not the definition (that is
tests/spliced_check.py).  Geometry, modes and end cells are those of tools/ends_model.py; costs = (go, ge, io, donor, acceptor, other)
as spliced_check.make_costs builds them, strand is +1 or -1.  With don(j) = start(j - 1) and acc(j) = end(j - 1) for the 1-based column
j, per row step and lane:

    F[k] = max(Hprev[k] - go, Fprev[k] - ge)                       lane-private; reads the true H
    T[k] = max(diag[k] + s, F[k])                                  H without a reference gap
    V    = max over k of T[k] - go + (p + 1) ge                    p = lane * cpl + k: the max-plus scan of E
    W    = max over k of X[k],  X[k] = T[k] - io - don(j + 1)      an intron costs nothing per letter: a plain prefix maximum
    e, u = exclusive prefix maxima of V and W over the lanes, lane 0 seeded with E and N of the chunk's first column
    along the lane  E[k] = e,  N[k] = u,  H[k] = max(T[k], E[k], N[k] - acc(j)),  e = max(e - ge, T[k] - go),  u = max(u, X[k])

io + don(j + 1) and acc(j) are set up once per chunk: a lane reads its own cpl letters, one before and two after them, so the
dinucleotides at a lane's and a chunk's edge take letters of the neighbour; a letter off the reference is code 4 and costs `other`.
Both strands' costs are tables over the dinucleotide as the reference reads it (`site_table`).  A chunk hands T, E and N of its last
column on, three values per row, and the next chunk rebuilds that column's H = max(T, E, N - acc).  With `store` a cell leaves one
byte: bits 0..1 H's source (0 diagonal, 1 E, 2 N, 3 F), bit 2 T's source (0 diagonal, 1 F), bits 3..5 "opened here" of E, N, F.
Every value a cell of the reference holds is checked to be an int32.

`fault` plants one wrong line (tests/test_spliced_host.py shows that each is caught):
    'donor_off'     the donor read one column off              'acc_at_open'  the acceptor paid at the opening, at the opening's column
    'handover_n'    N not handed to the next chunk             'open_from_h'  N opened from H and not from T
    'tie_flip'      N preferred over E on a tie                'minus_plain'  strand -: the tables not complemented
    'row0_plain'    row 0 without its intron"""
MODES = ('global', 'semiglobal', 'overlap', 'prefix', 'extend')
ANCHORED = ('global', 'prefix', 'extend')
FAULTS = ('donor_off', 'acc_at_open', 'handover_n', 'open_from_h', 'tie_flip', 'minus_plain', 'row0_plain')
OTHER = 64


def _i32(v):
    assert -(1 << 31) <= v < (1 << 31), v
    return v


def site_table(costs, fault=None):
    """65 costs: [0:16] start and [16:32] end of strand +, [32:48] and [48:64] of strand -, each by the dinucleotide 4 x + y as the
    reference reads it; [64] other (what clh_api.hip uploads)"""
    donor, acceptor, other = costs[3:]
    site = [0] * 65
    for x in range(4):
        for y in range(4):
            site[4 * x + y] = donor[4 * x + y]
            site[16 + 4 * x + y] = acceptor[4 * x + y]
            cx, cy = (x, y) if fault == 'minus_plain' else (3 - x, 3 - y)
            site[32 + 4 * x + y] = acceptor[4 * cy + cx]
            site[48 + 4 * x + y] = donor[4 * cy + cx]
    site[OTHER] = other
    return site


def run(q, r, mat, costs, mode, strand=1, cpl=8, lanes=64, store=True, fault=None):
    """-> the result dict of tests/ends_check.py (begins and cigar None without `store`)"""
    go, ge, io = costs[:3]
    assert mode in MODES and 0 <= ge <= go and io >= 0 and strand in (1, -1) and fault in (None,) + FAULTS
    m, n = len(q), len(r)
    assert m > 0 and n > 0, 'a pair with an empty side never reaches the kernel'
    site = site_table(costs, fault)
    soff = 32 if strand < 0 else 0

    def letter(pos):
        return int(r[pos]) if 0 <= pos < n else 4

    def cost(which, x, y):
        return site[OTHER if (x | y) > 3 else soff + which + 4 * x + y]

    def col0(i):
        return 0 if (mode == 'overlap' or i == 0) else -(go + (i - 1) * ge)
    iod1 = io + cost(0, letter(0), letter(1))

    def row0(j, a):
        if mode not in ANCHORED:
            return 0
        if fault == 'row0_plain':
            return -(go + (j - 1) * ge)
        return -min(go + (j - 1) * ge, iod1 + a)
    C = cpl * lanes
    nchunks = (n + C - 1) // C
    hand = [None, None]
    row_best, row_j = col0(m), 0
    col_best, col_i = 0, 0
    corner = None
    ext = [(0, 0, 0)] * lanes
    cells = {}
    shift = 1 if fault == 'donor_off' else 0
    for c in range(nchunks):
        c0 = c * C
        cols = min(C, n - c0)
        last = c == nchunks - 1
        iod_in = io + cost(0, letter(c0 + shift), letter(c0 + 1 + shift))
        acc_in = cost(16, letter(c0 - 2), letter(c0 - 1))
        iod = [[0] * cpl for _ in range(lanes)]
        acc = [[0] * cpl for _ in range(lanes)]
        for l in range(lanes):
            lt = [letter(c0 + l * cpl - 1 + t) for t in range(cpl + 4)]
            for k in range(cpl):
                iod[l][k] = io + cost(0, lt[k + 2 + shift], lt[k + 3 + shift])      # io + don(j + 1)
                acc[l][k] = cost(16, lt[k], lt[k + 1])                              # acc(j)
                if fault == 'acc_at_open':      # the close cost of the run's first column joins the opening, and leaving is free
                    iod[l][k] += cost(16, lt[k + 1], lt[k + 2])
        row0_acc = acc
        if fault == 'acc_at_open':
            iod_in += cost(16, letter(c0 - 1), letter(c0))
            acc1 = cost(16, letter(-1), letter(0))
            acc = [[0] * cpl for _ in range(lanes)]
            row0_acc = [[acc1] * cpl for _ in range(lanes)]
            h0_in = row0(c0, acc1) if c0 else 0
            acc_in = 0
        else:
            h0_in = row0(c0, acc_in) if c0 else 0
        Hp = [[row0(c0 + 1 + l * cpl + k, row0_acc[l][k]) for k in range(cpl)] for l in range(lanes)]
        Fp = [[h - go for h in Hp[l]] for l in range(lanes)]
        hleft = [Hp[l - 1][cpl - 1] if l else h0_in for l in range(lanes)]
        out = []
        ln, kn = (n - 1 - c0) // cpl, (n - 1 - c0) % cpl
        chunk_best = [None] * lanes
        for i in range(1, m + 1):
            if c == 0:
                tin = col0(i)
                hin, E0, N0 = tin, tin - go, tin - iod_in
            else:
                tin, ein, nin = hand[(c - 1) & 1][i - 1]
                hin = max(tin, ein, nin - acc_in)
                E0 = max(ein - ge, tin - go)
                N0 = tin - iod_in if fault == 'handover_n' else max(nin, tin - iod_in)
            T = [[0] * cpl for _ in range(lanes)]
            D = [[0] * cpl for _ in range(lanes)]
            F = [[0] * cpl for _ in range(lanes)]
            X = [[0] * cpl for _ in range(lanes)]
            VE, VN = [0] * lanes, [0] * lanes
            for l in range(lanes):
                ve = vn = None
                for k in range(cpl):
                    col = l * cpl + k
                    j = c0 + 1 + col
                    s = int(mat[r[j - 1]][q[i - 1]]) if j <= n else int(mat[0][q[i - 1]])
                    F[l][k] = max(Hp[l][k] - go, Fp[l][k] - ge)
                    D[l][k] = (Hp[l][k - 1] if k else hleft[l]) + s
                    T[l][k] = max(D[l][k], F[l][k])
                    X[l][k] = T[l][k] - iod[l][k]
                    xe = T[l][k] - go + (col + 1) * ge
                    ve = xe if ve is None or xe > ve else ve
                    vn = X[l][k] if vn is None or X[l][k] > vn else vn
                VE[l] = max(ve, E0) if l == 0 else ve
                VN[l] = max(vn, N0) if l == 0 else vn
            incE, incN = [], []
            for l in range(lanes):
                incE.append(VE[l] if not incE or VE[l] > incE[-1] else incE[-1])
                incN.append(VN[l] if not incN or VN[l] > incN[-1] else incN[-1])
            H = [[0] * cpl for _ in range(lanes)]
            E = [[0] * cpl for _ in range(lanes)]
            N = [[0] * cpl for _ in range(lanes)]
            for l in range(lanes):
                e = (incE[l - 1] if l else E0) - l * cpl * ge
                u = incN[l - 1] if l else N0
                for k in range(cpl):
                    if c0 + 1 + l * cpl + k <= n:
                        _i32(e + (l * cpl + k) * ge); _i32(u); _i32(T[l][k]); _i32(u - acc[l][k])
                    E[l][k], N[l][k] = e, u
                    H[l][k] = max(T[l][k], e, u - acc[l][k])
                    e = max(e - ge, T[l][k] - go)
                    u = max(u, (H[l][k] - iod[l][k]) if fault == 'open_from_h' else X[l][k])
            new_left = [H[l - 1][cpl - 1] if l else hin for l in range(lanes)]
            if store:
                for l in range((cols + cpl - 1) // cpl):
                    tleft = T[l - 1][cpl - 1] if l else tin
                    xleft = X[l - 1][cpl - 1] if l else tin - iod_in
                    for k in range(cpl):
                        tl = T[l][k - 1] if k else tleft
                        xl = X[l][k - 1] if k else xleft
                        h = H[l][k]
                        order = [D[l][k], E[l][k], N[l][k] - acc[l][k], F[l][k]]
                        src = order.index(h)
                        if fault == 'tie_flip' and h != D[l][k] and h == order[2]:
                            src = 2
                        b = src | (0 if T[l][k] == D[l][k] else 4)
                        b |= 8 if E[l][k] == tl - go else 0
                        b |= 16 if (N[l][k] == xl or (fault == 'open_from_h' and k and N[l][k] == H[l][k - 1] - iod[l][k - 1])) else 0
                        b |= 32 if F[l][k] == Hp[l][k] - go else 0
                        cells[(i, c0 + 1 + l * cpl + k)] = b
            if not last:
                out.append((T[lanes - 1][cpl - 1], E[lanes - 1][cpl - 1], N[lanes - 1][cpl - 1]))
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

    def row0_op(j):
        if fault == 'row0_plain':
            return 'D'
        d, x = go + (j - 1) * ge, iod1 + cost(16, letter(j - 2), letter(j - 1))
        return ('D' if d < x else 'N') if fault == 'tie_flip' else ('D' if d <= x else 'N')
    i0, j0, ops = walk(cells, mode, end, row0_op)
    res.update(ref_begin=j0, query_begin=i0, cigar=ops)
    return res


def walk(cells, mode, end, row0_op):
    """one lane walks the stored bytes back (pr_walk<EN_SPLICED> of csrc/ssw_pairs.h): states 0 H, 1 E, 2 N, 3 F, 4 T; every step consumes a
    letter, at most i + j + 2 steps.  (The kernel takes the cells of an E or N run that share a stored word in one step, up to the
    first "opened here" bit: the same cells in the same order.)"""
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
        if state in (0, 4) and (i == 0 or j == 0):
            if mode in ANCHORED:
                if j > 0:
                    emit(row0_op(j), j)
                emit('I', i); i = j = 0
            elif mode == 'semiglobal' and j == 0:
                emit('I', i); i = 0
            break
        b = cells[(i, j)]
        if state == 0:
            state = b & 3                    # a gap state takes its first letter from this same cell
            if state == 0:
                emit('M'); i -= 1; j -= 1
                continue
        elif state == 4:
            if not b & 4:
                emit('M'); i -= 1; j -= 1; state = 0
                continue
            state = 3
        if state == 1:
            emit('D'); j -= 1
            if b & 8:
                state = 4
        elif state == 2:
            emit('N'); j -= 1
            if b & 16:
                state = 4
        else:
            emit('I'); i -= 1
            if b & 32:
                state = 0
    else:
        raise AssertionError('the walk did not end')
    return i, j, [(o, k) for o, k in reversed(ops)]
