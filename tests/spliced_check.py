"""The definition of spliced pair alignment as ssw_wrap.align_pairs_spliced and clh_ends_plan_create_spliced state it (not a test
module): the full dynamic programme for the five modes of tests/ends_check.py and tests/anchored_check.py, its end cell, and the
walk back.

Sequences are DNA codes A, C, G, T = 0..3, anything else 4.  costs = (go, ge, io, donor, acceptor, other): a gap of k letters costs
go + (k - 1) ge, 0 <= ge <= go; io >= 0 opens an intron; donor[4 a + b] and acceptor[4 a + b] are 16 non-negative costs of the
dinucleotide (a, b) as read on the transcript strand; `other` is the cost of a dinucleotide that holds a code >= 4 or runs off the
reference.  `make_costs` builds the tuple.  strand is +1 or -1.

One rule: a maximal run of skipped reference letters r[a..b] (0-based, no query letter consumed in between) costs
min(go + (b - a) ge, io + start(a) + end(b)); insertions cost go + (k - 1) ge.
    strand +:  start(a) = donor[r[a], r[a+1]]                    end(b) = acceptor[r[b-1], r[b]]
    strand -:  start(a) = acceptor[c(r[a+1]), c(r[a])]           end(b) = donor[c(r[b]), c(r[b-1])]          c(x) = 3 - x
and `other` where a + 1 > n - 1 or b - 1 < 0.  The costs depend on the position alone: for a run of one letter the second letter of
the start dinucleotide lies outside the run.  In cells, 1-based columns, don(j) = start(j - 1), acc(j) = end(j - 1):

    F[i][j] = max(H[i-1][j] - go, F[i-1][j] - ge)            consumes a query letter (CIGAR I); reads the true H
    T[i][j] = max(H[i-1][j-1] + s(q_i, r_j), F[i][j])        H without a reference gap
    E[i][j] = max(T[i][j-1] - go, E[i][j-1] - ge)            a deletion (CIGAR D)
    N[i][j] = max(T[i][j-1] - io - don(j), N[i][j-1])        an intron (CIGAR N); the close cost is paid on leaving
    H[i][j] = max(T[i][j], E[i][j], N[i][j] - acc(j))

E and N open from T, not from H: a deletion run and an intron run are never adjacent, which makes the one rule exact
(tests/test_spliced_host.py holds `plain` to the enumeration of every alignment).  Boundaries, end cells and coordinates are those
of the one-piece checkers; row 0 of the anchored modes is what the recurrences give from T[0][0] = 0, H[0][j] = -min(go + (j - 1)
ge, io + don(1) + acc(j)); column 0 is unchanged and T[i][0] is the F boundary.  The walk prefers, in state H, the diagonal, then E,
then N, then F; in state E it emits D, moves left and leaves as soon as E[i][j] == T[i][j-1] - go (N likewise with N[i][j] ==
T[i][j-1] - io - don(j), emitting N); on leaving E or N it is in state T: the diagonal if T equals it, else F.  The anchored stop on
row 0 at column j > 0 emits one run of j letters, D if the deletion is not dearer, else N.

`plain` is the recurrence cell by cell in Python integers; `align` builds each row with numpy for the larger GPU cases.
`check_cigar` costs every maximal D run as a deletion and every N run as an intron, with no knowledge of tie rules."""
import numpy as np

import anchored_check as ac
import ends_check as ec

MODES = ec.MODES + ac.MODES
NEG = ec.NEG

rng_for = ec.rng_for
dna_matrix = ec.dna_matrix
encode = ec.encode
random_seq = ec.random_seq
mutate = ec.mutate
parse_cigar = ec.parse_cigar
as_tuple = ec.as_tuple
cigar_text = ec.cigar_text


def make_costs(go=3, ge=1, io=12, noncanonical=6, donor=None, acceptor=None):
    """the tuple the functions here take: GT and AG cost 0, every other dinucleotide and `other` cost noncanonical; the dicts
    override single dinucleotides, e.g. {'GC': 2}"""
    def table(free, over):
        t = [int(noncanonical)] * 16
        t[4 * 'ACGT'.index(free[0]) + 'ACGT'.index(free[1])] = 0
        for key, v in (over or {}).items():
            t[4 * 'ACGT'.index(key[0]) + 'ACGT'.index(key[1])] = int(v)
        return tuple(t)
    return (int(go), int(ge), int(io), table('GT', donor), table('AG', acceptor), int(noncanonical))


def violated(costs):
    go, ge, io, donor, acceptor, other = costs
    if not 0 <= ge <= go:
        return '0 <= gap_extend <= gap_open'
    if io < 0 or other < 0 or min(donor) < 0 or min(acceptor) < 0:
        return 'intron costs >= 0'
    return None


def _di(table, other, a, b):
    return other if a > 3 or b > 3 else table[4 * a + b]


def site_costs(r, costs, strand):
    """-> (don, acc): lists of n + 1 values, don[j] = start(j - 1) and acc[j] = end(j - 1) for the 1-based column j (index 0 unused)"""
    assert strand in (1, -1)
    _, _, _, donor, acceptor, other = costs
    n = len(r)
    r = [int(x) for x in r]
    don, acc = [None] * (n + 1), [None] * (n + 1)
    for j in range(1, n + 1):
        a = b = j - 1
        if strand > 0:
            don[j] = _di(donor, other, r[a], r[a + 1]) if a + 1 <= n - 1 else other
            acc[j] = _di(acceptor, other, r[b - 1], r[b]) if b - 1 >= 0 else other
        else:
            don[j] = _di(acceptor, other, 3 - r[a + 1] if r[a + 1] < 4 else 4, 3 - r[a] if r[a] < 4 else 4) if a + 1 <= n - 1 else other
            acc[j] = _di(donor, other, 3 - r[b] if r[b] < 4 else 4, 3 - r[b - 1] if r[b - 1] < 4 else 4) if b - 1 >= 0 else other
    return don, acc


def run_costs(a, b, costs, don, acc):
    """(as a deletion, as an intron) of the skipped reference letters r[a..b], 0-based"""
    go, ge, io = costs[:3]
    return go + (b - a) * ge, io + don[a + 1] + acc[b + 1]


def _anchored(mode):
    return mode in ('global', 'prefix', 'extend')


def _end_cell(mode, m, n, H):
    if mode in ec.MODES:
        return ec._end_cell(mode, m, n, [H(m, j) for j in range(n + 1)], [H(i, n) for i in range(m + 1)])
    return ac._end_cell(mode, m, n, [(i, j, H(i, j)) for i in range(m + 1) for j in range(n + 1)])[:2]


def _walk(mode, end, src, tsrc, opened, row0_op):
    """src(i, j): 0 diagonal, 1 E, 2 N, 3 F, the first that equals H; tsrc(i, j): 0 where T is the diagonal, else 1 (F); opened(i, j,
    s): state s (1 E, 2 N, 3 F) leaves its run at (i, j); row0_op(j): the op of the run of j letters on row 0"""
    i, j = end
    ops = []

    def emit(op, k=1):
        if k <= 0:
            return
        if ops and ops[-1][0] == op:
            ops[-1][1] += k
        else:
            ops.append([op, k])
    state = 'H'
    while True:
        if state in 'HT' and (i == 0 or j == 0):        # on column 0 T is H; the walk is never in state T on row 0
            assert state == 'H' or i > 0
            if _anchored(mode):
                if j:
                    emit(row0_op(j), j)
                emit('I', i)
                i = j = 0
            elif mode == 'semiglobal' and j == 0:
                emit('I', i); i = 0
            break
        if state == 'H':
            s = src(i, j)
            if s == 0:
                emit('M'); i -= 1; j -= 1
            else:
                state = ' ENF'[s]
        elif state == 'T':
            if tsrc(i, j) == 0:
                emit('M'); i -= 1; j -= 1
                state = 'H'
            else:
                state = 'F'
        elif state == 'E':
            emit('D')
            if opened(i, j, 1):
                state = 'T'
            j -= 1
        elif state == 'N':
            emit('N')
            if opened(i, j, 2):
                state = 'T'
            j -= 1
        else:
            emit('I')
            if opened(i, j, 3):
                state = 'H'
            i -= 1
    return i, j, [(o, k) for o, k in reversed(ops)]


def _row0_op(costs, don, acc):
    def op(j):
        d, x = run_costs(0, j - 1, costs, don, acc)
        return 'D' if d <= x else 'N'
    return op


def plain(q, r, mat, costs, mode, strand=1):
    """the recurrence, one cell after the other, in Python integers"""
    assert mode in MODES and violated(costs) is None
    go, ge, io = costs[:3]
    m, n = len(q), len(r)
    don, acc = site_costs(r, costs, strand)
    H = [[NEG] * (n + 1) for _ in range(m + 1)]
    T = [[NEG] * (n + 1) for _ in range(m + 1)]
    D = [[NEG] * (n + 1) for _ in range(m + 1)]
    E = [[NEG] * (n + 1) for _ in range(m + 1)]
    N = [[NEG] * (n + 1) for _ in range(m + 1)]
    F = [[NEG] * (n + 1) for _ in range(m + 1)]
    H[0][0] = T[0][0] = 0
    for j in range(1, n + 1):
        if _anchored(mode):
            E[0][j] = max(T[0][j - 1] - go, E[0][j - 1] - ge)
            N[0][j] = max(T[0][j - 1] - io - don[j], N[0][j - 1])
            H[0][j] = max(E[0][j], N[0][j] - acc[j])
        else:
            H[0][j] = T[0][j] = 0
    for i in range(1, m + 1):
        if mode == 'overlap':
            H[i][0] = T[i][0] = 0
        else:
            F[i][0] = max(H[i - 1][0] - go, F[i - 1][0] - ge)
            H[i][0] = T[i][0] = F[i][0]
    for i in range(1, m + 1):
        for j in range(1, n + 1):
            F[i][j] = max(H[i - 1][j] - go, F[i - 1][j] - ge)
            D[i][j] = H[i - 1][j - 1] + int(mat[r[j - 1]][q[i - 1]])
            T[i][j] = max(D[i][j], F[i][j])
            E[i][j] = max(T[i][j - 1] - go, E[i][j - 1] - ge)
            N[i][j] = max(T[i][j - 1] - io - don[j], N[i][j - 1])
            H[i][j] = max(T[i][j], E[i][j], N[i][j] - acc[j])
    end = _end_cell(mode, m, n, lambda i, j: H[i][j])

    def src(i, j):
        return [D[i][j], E[i][j], N[i][j] - acc[j], F[i][j]].index(H[i][j])

    def opened(i, j, s):
        if s == 1:
            return E[i][j] == T[i][j - 1] - go
        if s == 2:
            return N[i][j] == T[i][j - 1] - io - don[j]
        return F[i][j] == H[i - 1][j] - go
    i0, j0, ops = _walk(mode, end, src, lambda i, j: 0 if T[i][j] == D[i][j] else 1, opened, _row0_op(costs, don, acc))
    return ec._result(H[end[0]][end[1]], end, (i0, j0), ops)


def align(q, r, mat, costs, mode, strand=1, path=True):
    """the same programme row by row in numpy int64; path=False: score and end cell only (begins and cigar None)"""
    assert mode in MODES and violated(costs) is None
    go, ge, io = costs[:3]
    q = np.asarray(q, dtype=np.int64); r = np.asarray(r, dtype=np.int64)
    mat = np.asarray(mat, dtype=np.int64)
    m, n = len(q), len(r)
    dl, al = site_costs(r, costs, strand)
    don = np.array([0] + dl[1:], dtype=np.int64); acc = np.array([0] + al[1:], dtype=np.int64)
    ar = np.arange(n + 1, dtype=np.int64) * ge
    if _anchored(mode) and n:
        Hp = np.concatenate([[0], -np.minimum(go + ar[:-1], io + don[1] + acc[1:])]).astype(np.int64)
    else:
        Hp = np.zeros(n + 1, dtype=np.int64)
    col0 = [0] + [0 if mode == 'overlap' else -(go + (i - 1) * ge) for i in range(1, m + 1)]
    Fp = np.full(n + 1, NEG, dtype=np.int64)
    flags = np.zeros((m + 1, n + 1), dtype=np.uint8) if path else None      # bits 0..1 H's source, 2 T's source, 3..5 opened here: E, N, F
    last_col = [int(Hp[n])]
    best = (0, 0, 0)                                                        # extend: (i, j, H), the first of the greatest in row order
    for i in range(1, m + 1):
        F = np.maximum(Hp - go, Fp - ge)
        T = np.empty(n + 1, dtype=np.int64)
        T[0] = col0[i]
        d = Hp[:-1] + mat[r, q[i - 1]] if n else np.zeros(0, dtype=np.int64)
        T[1:] = np.maximum(d, F[1:])
        E = np.full(n + 1, NEG, dtype=np.int64)
        N = np.full(n + 1, NEG, dtype=np.int64)
        H = T.copy()
        if n:
            E[1:] = np.maximum.accumulate(T[:-1] - go + ar[1:]) - ar[1:]
            N[1:] = np.maximum.accumulate(T[:-1] - io - don[1:])
            H[1:] = np.maximum(T[1:], np.maximum(E[1:], N[1:] - acc[1:]))
        if path and n:
            h = H[1:]
            s = np.where(h == d, 0, np.where(h == E[1:], 1, np.where(h == N[1:] - acc[1:], 2, 3))).astype(np.uint8)
            assert ((s < 3) | (h == F[1:])).all()
            s |= (T[1:] != d).astype(np.uint8) << 2
            s |= (E[1:] == T[:-1] - go).astype(np.uint8) << 3
            s |= (N[1:] == T[:-1] - io - don[1:]).astype(np.uint8) << 4
            s |= (F[1:] == Hp[1:] - go).astype(np.uint8) << 5
            flags[i, 1:] = s
        Hp, Fp = H, F
        Fp[0] = NEG if mode == 'overlap' else col0[i]
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
    i0, j0, ops = _walk(mode, end, lambda i, j: int(flags[i, j]) & 3, lambda i, j: (int(flags[i, j]) >> 2) & 1,
                        lambda i, j, s: (int(flags[i, j]) >> (2 + s)) & 1, _row0_op(costs, dl, al))
    return ec._result(score, end, (i0, j0), ops)


def rescore(cigar, q, r, ref_begin, query_begin, mat, costs, strand=1):
    """what a CIGAR costs, read from left to right with no knowledge of how it was chosen: every run of D as a deletion, every run
    of N as an intron at its own position -> (score, reference letters, query letters)"""
    go, ge = costs[:2]
    don, acc = site_costs(r, costs, strand)
    i, j, score = query_begin, ref_begin, 0
    for op, k in cigar:
        assert k > 0
        if op == 'M':
            for _ in range(k):
                score += int(mat[r[j]][q[i]]); i += 1; j += 1
        elif op == 'I':
            score -= go + (k - 1) * ge; i += k
        else:
            assert op in 'DN', op
            score -= run_costs(j, j + k - 1, costs, don, acc)[op == 'N']; j += k
    return score, j - ref_begin, i - query_begin


def check_cigar(res, q, r, mat, costs, mode, strand=1):
    """the CIGAR of a result rescores to its score and spans exactly its coordinates; no D stands next to an N; the spans are what
    the mode allows"""
    m, n = len(q), len(r)
    score, nr, nq = rescore(res['cigar'], q, r, res['ref_begin'], res['query_begin'], mat, costs, strand)
    assert score == res['score'], (score, res)
    assert res['ref_begin'] + nr - 1 == res['ref_end'] and res['query_begin'] + nq - 1 == res['query_end'], (nr, nq, res)
    assert 0 <= res['ref_begin'] <= res['ref_end'] + 1 <= n and 0 <= res['query_begin'] <= res['query_end'] + 1 <= m, res
    ops = [o for o, _ in res['cigar']]
    assert all(a != b and {a, b} != {'D', 'N'} for a, b in zip(ops, ops[1:])), res['cigar']
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
