"""Python model of K4m / K4t (csrc/edit_align.hip): K4's Myers/Hyyro blocks of 64 query rows per mode, the last-row
tracking that gives the best score and every optimal column, the reverse SHW passes that give HW starts, and the traceback
from stored per-block vectors (Pv, Mv and the block's bottom score per column).  Pure Python, small cases; it states the
recurrences the kernels use.  tests/edlib_check.py is the plain dynamic programme it is tested against."""
M64 = (1 << 64) - 1


def _peq(pat, partners):
    """match vectors per block: letter -> bit mask of the block's rows that equal it (or one of its partners)"""
    B = (len(pat) + 63) // 64
    peq = [dict() for _ in range(B)]
    for r, c in enumerate(pat):
        for d in [c] + partners.get(c, []):
            peq[r >> 6][d] = peq[r >> 6].get(d, 0) | (1 << (r & 63))
    return peq


def blocks(pat, txt, hin0, partners=None, store=False):
    """one sweep of the text over the pattern's blocks.  hin0: horizontal delta entering block 0 (+1 NW/SHW, 0 HW).
    -> (last-row score per column, stored [(Pv, Mv, bottom score) per block] per column if store)"""
    m = len(pat)
    B = (m + 63) // 64
    peq = _peq(pat, partners or {})
    Pv, Mv = [M64] * B, [0] * B
    rows = [min(64, m - 64 * b) for b in range(B)]
    bottom = [64 * b + rows[b] for b in range(B)]       # the block's bottom row in column -1
    last, stored = [], []
    for c in txt:
        hin = hin0
        col = []
        for b in range(B):
            lb = rows[b] - 1
            Eq = peq[b].get(c, 0)
            Xv = Eq | Mv[b]
            if hin < 0:
                Eq |= 1
            Xh = ((((Eq & Pv[b]) + Pv[b]) & M64) ^ Pv[b]) | Eq
            Ph = (Mv[b] | ~(Xh | Pv[b])) & M64
            Mh = Pv[b] & Xh
            bottom[b] += ((Ph >> lb) & 1) - ((Mh >> lb) & 1)
            hout = ((Ph >> 63) & 1) - ((Mh >> 63) & 1)
            Ph = (Ph << 1) & M64
            Mh = (Mh << 1) & M64
            if hin < 0:
                Mh |= 1
            elif hin > 0:
                Ph |= 1
            Pv[b] = (Mh | ~(Xv | Ph)) & M64
            Mv[b] = Ph & Xv
            hin = hout
            if store:
                col.append((Pv[b], Mv[b], bottom[b]))
        last.append(bottom[B - 1])
        if store:
            stored.append(col)
    return last, stored


def score_pass(q, t, mode, partners=None):
    """K4m: best last-row score and the optimal columns (HW: column -1 first, score m)"""
    last, _ = blocks(q, t, 0 if mode == 'HW' else 1, partners)
    if mode == 'NW':
        return last[-1], [len(t) - 1]
    best, ends = (len(q), [-1]) if mode == 'HW' else (None, [])
    for col, s in enumerate(last):
        if best is None or s < best:
            best, ends = s, [col]
        elif s == best:
            ends.append(col)
    return best, ends


def reverse_pass(q, t, end, best, partners=None):
    """SHW of the reversed query over target[end], target[end-1], ... for at most m + best + 1 columns: the last optimal
    position p -> start = end - p"""
    P = min(end + 1, len(q) + best + 1)
    last, _ = blocks(q[::-1], [t[end - x] for x in range(P)], 1, partners)
    b = min(last)
    return end - max(p for p, s in enumerate(last) if s == b)


def H(stored, i, j):
    """D[i][j] of the NW matrix from the stored vectors of column j - 1: the bottom score of the block above plus the
    vertical deltas of rows 0..r of the block"""
    if i == 0:
        return j
    if j == 0:
        return i
    b, r = (i - 1) >> 6, (i - 1) & 63
    Pv, Mv, _ = stored[j - 1][b]
    mask = (2 << r) - 1
    base = j if b == 0 else stored[j - 1][b - 1][2]
    return base + bin(Pv & mask).count('1') - bin(Mv & mask).count('1')


def path(q, t, eq):
    """K4t: NW with stored vectors, then the walk back (I, then D, then the diagonal) -> [(op, length)]"""
    partners = {}
    for a, b in eq:
        if a != b:
            partners.setdefault(a, []).append(b)
            partners.setdefault(b, []).append(a)
    m, L = len(q), len(t)
    stored = blocks(q, t, 1, partners, store=True)[1] if m and L else []
    i, j, ops = m, L, []
    while i > 0 or j > 0:
        h = H(stored, i, j)
        if i > 0 and H(stored, i - 1, j) + 1 == h:
            o = 'I'; i -= 1
        elif j > 0 and H(stored, i, j - 1) + 1 == h:
            o = 'D'; j -= 1
        else:
            a, c = q[i - 1], t[j - 1]
            o = '=' if a == c or c in partners.get(a, []) else 'X'; i -= 1; j -= 1
        if ops and ops[-1][0] == o:
            ops[-1][1] += 1
        else:
            ops.append([o, 1])
    return [(o, n) for o, n in reversed(ops)]


def align(query, target, mode='NW', task='distance', k=-1, eq=()):
    """the result dict of ciri_long_amd.edlib.align, from the block passes (strings as bytes or lists of ints)"""
    q, t = list(bytes(query)), list(bytes(target))
    partners = {}
    for a, b in eq:
        if a != b:
            partners.setdefault(a, []).append(b)
            partners.setdefault(b, []).append(a)
    m, n = len(q), len(t)
    if m == 0 or n == 0:           # the empty sides are stated by the host, not the kernels
        if n == 0:
            best, ends = m, [-1]
        elif mode == 'NW':
            best, ends = n, [n - 1]
        elif mode == 'SHW':
            best, ends = 1, [0]
        else:
            best, ends = 0, list(range(-1, n))
    else:
        best, ends = score_pass(q, t, mode, partners)
    alpha = len(set(q) | set(t))
    if k >= 0 and best > k:
        return {'editDistance': -1, 'alphabetLength': alpha, 'locations': [], 'cigar': None}
    if task == 'distance':
        locs = [(None, e) for e in ends]
    elif mode == 'HW':
        locs = [((e + 1) if m == 0 else 0 if e < 0 else reverse_pass(q, t, e, best, partners), e) for e in ends]
    else:
        locs = [(0, e) for e in ends]
    cigar = None
    if task == 'path':
        s, e = locs[0]
        cigar = ''.join('%d%s' % (nn, o) for o, nn in path(q, t[s:e + 1], eq))
    return {'editDistance': best, 'alphabetLength': alpha, 'locations': locs, 'cigar': cigar}
