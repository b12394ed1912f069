"""Python model of K4s (csrc/edit_search.hip): a probe of one Myers word searched in a text (edlib's HW mode, task
"locations") by column segments that start afresh.

Segment s owns the columns [s SEG, (s + 1) SEG).  Its recurrence starts 2 m columns earlier (clamped at 0) from the HW initial
state -- top row 0, Pv all ones, score m -- walks the warm-up without counting it, then keeps over its owned columns the tuple
(best, first column, last column, count).  Why that is exact: an alignment of cost d covers at most m + d target columns and
the best cost at any column is at most m, so every alignment that decides the last-row value of an owned column starts inside
the warm-up, and a fresh start can only raise values.  Tuples join by the minimum best and, among its holders, the minimum
first, the maximum last and the sum of counts; the join is seeded with column -1 at score m.  In the kernel, segment s is lane
s % 64 of round s // 64, and rounds are dealt to waves in chunks; none of that changes the tuples.  The start of the first
location is align's rule: SHW of the reversed probe over the reversed text[.. end], at most m + best + 1 columns, the last
optimal position.  Pure Python, small cases; tests/edlib_check.py is the plain dynamic programme it is tested against."""
NONE = (1 << 31) - 1


def peq_of(probe, eq=()):
    """letter -> bit mask of the probe's rows that equal it or are paired with it (symmetric, not transitive)"""
    peq = {}
    for r, c in enumerate(probe):
        peq[c] = peq.get(c, 0) | (1 << r)
        for a, b in eq:
            if c == a:
                peq[b] = peq.get(b, 0) | (1 << r)
            if c == b:
                peq[a] = peq.get(a, 0) | (1 << r)
    return peq


def step(Eq, Pv, Mv, m, hin):
    """one column of Myers/Hyyro on one word of m rows; hin: the delta entering row 0 (0 HW, 1 SHW) -> (Pv, Mv, last row's delta)"""
    mask = (1 << m) - 1
    Xv = Eq | Mv
    Xh = ((((Eq & Pv) + Pv) & mask) ^ Pv) | Eq
    Ph = (Mv | ~(Xh | Pv)) & mask
    Mh = Pv & Xh
    d = ((Ph >> (m - 1)) & 1) - ((Mh >> (m - 1)) & 1)
    Ph = ((Ph << 1) | hin) & mask
    Mh = (Mh << 1) & mask
    return (Mh | ~(Xv | Ph)) & mask, Ph & Xv, d


def join(a, b):
    if b[0] < a[0]:
        return b
    if b[0] > a[0]:
        return a
    return (a[0], min(a[1], b[1]), max(a[2], b[2]), a[3] + b[3])


def segment(probe, text, peq, s, seg):
    """the tuple of segment s: fresh start 2 m columns before its first owned column, warm-up walked and not counted"""
    m, n = len(probe), len(text)
    own0 = s * seg
    tup = (NONE, NONE, -2, 0)
    if own0 >= n:
        return tup
    Pv, Mv, score = (1 << m) - 1, 0, m
    for col in range(max(0, own0 - 2 * m), min(own0 + seg, n)):
        Pv, Mv, d = step(peq.get(text[col], 0), Pv, Mv, m, 0)
        score += d
        if col >= own0:
            tup = join(tup, (score, col, col, 1))
    return tup


def start_of(probe, text, end, best, peq):
    """SHW of the reversed probe over text[end], text[end - 1], ... for at most m + best + 1 columns -> end - last optimal position"""
    m = len(probe)
    rev = {c: int(format(v, '0%db' % m)[::-1], 2) for c, v in peq.items()}
    Pv, Mv, score, last = (1 << m) - 1, 0, m, None
    for x in range(min(end + 1, m + best + 1)):
        Pv, Mv, d = step(rev.get(text[end - x], 0), Pv, Mv, m, 1)
        score += d
        if score == best:
            last = x
    return end - last


def search(probe, text, seg, k=-1, eq=()):
    """(distance, start, end, last_end, nlocs) of one cell, as ciri_long_amd.edlib.search defines it; probe of 1..64 letters"""
    probe, text = list(bytes(probe)), list(bytes(text))
    m, n = len(probe), len(text)
    assert 1 <= m <= 64 and seg >= 1
    peq = peq_of(probe, eq)
    tup = (m, -1, -1, 1)                                   # column -1: the probe in front of the text
    for s in range((n + seg - 1) // seg):
        tup = join(tup, segment(probe, text, peq, s, seg))
    best, first, last, cnt = tup
    if k >= 0 and best > k:
        return (-1, -2, -2, -2, 0)
    return (best, 0 if first < 0 else start_of(probe, text, first, best, peq), first, last, cnt)
