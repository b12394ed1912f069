"""numpy statement of edlib.align as ciri_long_amd.edlib defines it (not a test module): every field of the result dict
derived from the plain dynamic programme, one row at a time with the row trick

    D[i][j] = min over j' <= j of (T[j'] + j - j'),  T[j] = min(D[i-1][j] + 1, D[i-1][j-1] + cost),  T[0] = i
            = np.minimum.accumulate(T - arange) + arange

D[i][j]: query[0..i) against j target letters (column j - 1 of the target; j = 0 is column -1, before the target).
Row 0 is j for NW and SHW and 0 for HW."""
import numpy as np


def _arr(s):
    if isinstance(s, str):
        s = s.encode('latin-1')
    return np.frombuffer(bytes(s), dtype=np.uint8)


def eq_matrix(equalities=None):
    m = np.eye(256, dtype=bool)
    for a, b in equalities or ():
        a = a if isinstance(a, int) else _arr(a)[0]
        b = b if isinstance(b, int) else _arr(b)[0]
        m[a, b] = m[b, a] = True
    return m


def rows(q, t, mode, eqm):
    """yields D[0], D[1], ... D[m] (int64 arrays of n + 1)"""
    n = len(t)
    ar = np.arange(n + 1, dtype=np.int64)
    row = ar.copy() if mode in ('NW', 'SHW') else np.zeros(n + 1, dtype=np.int64)
    yield row
    for i in range(1, len(q) + 1):
        cost = (~eqm[q[i - 1]][t]).astype(np.int64)
        T = np.empty(n + 1, dtype=np.int64)
        T[0] = i
        T[1:] = np.minimum(row[1:] + 1, row[:-1] + cost)
        row = np.minimum.accumulate(T - ar) + ar
        yield row


def last_row(q, t, mode, eqm):
    r = None
    for r in rows(q, t, mode, eqm):
        pass
    return r


def candidates(mode, n):
    """the j of D[m][j] an alignment of the mode may end at"""
    if mode == 'NW' or n == 0:
        return np.array([n])
    if mode == 'SHW':
        return np.arange(1, n + 1)
    return np.arange(0, n + 1)


def ends_of(q, t, mode, eqm):
    last = last_row(q, t, mode, eqm)
    cand = candidates(mode, len(t))
    best = int(last[cand].min())
    return best, [int(j) - 1 for j in cand if last[j] == best]


def hw_start(q, t, end, best, eqm):
    """SHW of the reversed query over the reversed target[0..end], bounded to m + best + 1 columns; the last optimal
    position p gives start = end - p"""
    if len(q) == 0:
        return end + 1
    if end < 0:
        return 0
    P = min(end + 1, len(q) + best + 1)
    rt = t[:end + 1][::-1][:P]
    last = last_row(q[::-1], rt, 'SHW', eqm)
    b = int(last[1:].min())
    assert b == best, (b, best)
    p = max(j - 1 for j in range(1, P + 1) if last[j] == b)
    return end - p


def nw_matrix(q, t, eqm):
    return np.array(list(rows(q, t, 'NW', eqm)), dtype=np.int64)


def traceback(q, t, eqm):
    """NW path of q against t by the tie rule: I if H[i-1][j] + 1 == H[i][j], else D if H[i][j-1] + 1 == H[i][j], else the
    diagonal (= or X) -> list of (op, length), op in '=XID'"""
    H = nw_matrix(q, t, eqm)
    i, j = len(q), len(t)
    ops = []
    while i > 0 or j > 0:
        if i > 0 and H[i - 1, j] + 1 == H[i, j]:
            o = 'I'; i -= 1
        elif j > 0 and H[i, j - 1] + 1 == H[i, j]:
            o = 'D'; j -= 1
        else:
            assert i > 0 and j > 0 and H[i - 1, j - 1] + (0 if eqm[q[i - 1], t[j - 1]] else 1) == H[i, j]
            o = '=' if eqm[q[i - 1], t[j - 1]] else 'X'; i -= 1; j -= 1
        if ops and ops[-1][0] == o:
            ops[-1][1] += 1
        else:
            ops.append([o, 1])
    return [(o, n) for o, n in reversed(ops)]


def cigar_text(ops):
    return ''.join('%d%s' % (n, o) for o, n in ops)


def parse_cigar(c):
    out, num = [], ''
    for ch in c:
        if ch.isdigit():
            num += ch
        else:
            out.append((ch, int(num))); num = ''
    return out


def align(query, target, mode='NW', task='distance', k=-1, additionalEqualities=None):
    """the result dict ciri_long_amd.edlib.align returns"""
    q, t = _arr(query), _arr(target)
    eqm = eq_matrix(additionalEqualities)
    best, ends = ends_of(q, t, mode, eqm)
    alpha = len(set(q.tolist()) | set(t.tolist()))
    if k >= 0 and best > k:
        return {'editDistance': -1, 'alphabetLength': alpha, 'locations': [], 'cigar': None}
    if task == 'distance':
        locs = [(None, e) for e in ends]
    elif mode == 'HW':
        locs = [(hw_start(q, t, e, best, eqm), e) for e in ends]
    else:
        locs = [(0, e) for e in ends]
    cigar = None
    if task == 'path':
        s, e = locs[0]
        cigar = cigar_text(traceback(q, t[s:e + 1], eqm))
    return {'editDistance': best, 'alphabetLength': alpha, 'locations': locs, 'cigar': cigar}


def bounded(res, k):
    """align()'s k rule applied to a free (k = -1) result: a best above k leaves the empty result"""
    if k >= 0 and res['editDistance'] > k:
        return {'editDistance': -1, 'alphabetLength': res['alphabetLength'], 'locations': [], 'cigar': None}
    return res


def suffix_distances(q, t, lo, e, eqm):
    """NW distance of q against target[s..e] for every s in lo .. e + 1 (at index s - lo), from one programme over the reversed
    strings.  This is the reverse pass's own idea (hw_start), so check_locations uses it as a cross-check only."""
    return last_row(q[::-1], t[lo:e + 1][::-1], 'NW', eqm)[::-1]


def nw_distance(q, t, eqm, w=None):
    """forward NW distance of q against t.  With a band w: the distance when it is <= w, else w + 1 -- an alignment of cost
    <= w never leaves the diagonals |j - i| <= w, and cells outside them count as unreachable (which can only raise a value)"""
    m, L = len(q), len(t)
    if w is None or w >= max(m, L):
        return int(last_row(q, t, 'NW', eqm)[-1])
    if abs(L - m) > w:
        return w + 1
    INF = 1 << 40
    row = np.full(L + 1, INF, dtype=np.int64)
    row[:min(L, w) + 1] = np.arange(min(L, w) + 1)
    for i in range(1, m + 1):
        lo, hi = max(0, i - w), min(L, i + w)          # the columns of row i inside the band
        T = row[lo:hi + 1] + 1
        if lo == 0:
            T[0] = i
            if hi >= 1:
                T[1:] = np.minimum(T[1:], row[0:hi] + ~eqm[q[i - 1]][t[0:hi]])
        else:
            T = np.minimum(T, row[lo - 1:hi] + ~eqm[q[i - 1]][t[lo - 1:hi]])
            row[lo - 1] = INF                          # column lo - 1 has left the band
        ar = np.arange(hi - lo + 1)
        row[lo:hi + 1] = np.minimum.accumulate(T - ar) + ar
    return int(min(row[L], w + 1))


def check_locations(res, query, target, mode, additionalEqualities=None, seed=0):
    """What a location is, stated forwards and without the reverse pass.  For every location (s, e) with a start, the NW distance
    of the query against target[s..e] -- one forward programme on that slice -- is editDistance.  For HW, no s' < s has that
    property (s is the smallest start, the longest alignment): one forward programme per candidate s', with two facts that spare
    programmes and use no reversed string.  A slice of more than m + editDistance letters costs more than editDistance, so the
    search starts at e + 1 - m - editDistance.  One target letter more or fewer changes an NW distance by at most 1, so a
    candidate s' whose slice costs editDistance + g rules out every s'' with |s'' - s'| < g, and the search steps down by g; the
    candidate's programme is banded (nw_distance), which caps g.  Pairs of m * n <= 2**12 are searched at every s' from s - 1
    down to 0, unbanded, without either fact.  The smallest-start half is applied to every location when m * n <= 2**22, and to
    the first, the last and two seeded others above that.  Last, as a cross-check only, the one-programme reversed form
    (suffix_distances) must agree.  -> the number of locations proved in full"""
    import random
    q, t = _arr(query), _arr(target)
    eqm = eq_matrix(additionalEqualities)
    d, locs = res['editDistance'], [(s, e) for s, e in res['locations'] if s is not None]
    if d < 0 or not locs:
        return 0
    m, n = len(q), len(t)
    full = set(range(len(locs)))
    if mode == 'HW' and m * n > 2 ** 22 and len(locs) > 4:
        full = {0, len(locs) - 1} | set(random.Random(seed).sample(range(1, len(locs) - 1), 2))
    proved = 0
    for x, (s, e) in enumerate(locs):
        assert 0 <= s <= e + 1 <= n, (s, e)
        assert nw_distance(q, t[s:e + 1], eqm) == d, (s, e, d)
        if mode != 'HW':
            assert s == 0
            proved += 1
            continue
        if x not in full:
            continue
        if m * n <= 2 ** 12:
            for s2 in range(s):
                assert nw_distance(q, t[s2:e + 1], eqm) != d, (s, e, 'a smaller start has the same distance', s2)
        else:
            lo, s2, w = max(0, e + 1 - m - d), s - 1, d + 64
            assert lo <= s, (s, e, 'a slice of more than m + editDistance letters')
            while s2 >= lo:
                g = nw_distance(q, t[s2:e + 1], eqm, w) - d
                assert g != 0, (s, e, 'a smaller start has the same distance', s2)
                assert g > 0, (s, e, s2, 'a slice below the best distance')
                s2 -= g
        lo = max(0, e + 1 - m - d)
        dist = suffix_distances(q, t, lo, e, eqm)
        assert dist[s - lo] == d and not (dist[:s - lo] == d).any(), (s, e, 'the reversed programme disagrees')
        proved += 1
    return proved


def check_invariants(res, query, target, mode, additionalEqualities=None):
    """the CIGAR costs editDistance and consumes exactly the query and target[start..end]; ends are ascending and allowed"""
    q, t = _arr(query), _arr(target)
    eqm = eq_matrix(additionalEqualities)
    if res['editDistance'] < 0:
        assert res['locations'] == [] and res['cigar'] is None
        return
    ends = [e for _, e in res['locations']]
    assert ends == sorted(ends) and len(set(ends)) == len(ends)
    for s, e in res['locations']:
        assert -1 <= e < max(len(t), 0) or (e == -1 and len(t) == 0)
        if mode == 'NW':
            assert e == len(t) - 1
        if s is not None:
            assert 0 <= s <= e + 1
    if res['cigar'] is None:
        return
    s, e = res['locations'][0]
    qi, ti, cost = 0, s, 0
    for o, n in parse_cigar(res['cigar']):
        for _ in range(n):
            if o in '=X':
                assert bool(eqm[q[qi], t[ti]]) == (o == '='), (o, qi, ti)
                cost += o == 'X'; qi += 1; ti += 1
            elif o == 'I':
                cost += 1; qi += 1
            else:
                assert o == 'D'
                cost += 1; ti += 1
    assert qi == len(q) and ti == e + 1, (qi, ti, len(q), e)
    assert cost == res['editDistance']
