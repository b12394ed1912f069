"""The definition of end-anchored affine-gap alignment of a pair (modes global, semiglobal, overlap) as ssw_wrap.align_pairs_ends
and clh_ends_* state it (not a test module): the full dynamic programme in int64, its end cell, and the walk back.

    E[i][j] = max(H[i][j-1] - go, E[i][j-1] - ge)      consumes a reference letter   (CIGAR D)
    F[i][j] = max(H[i-1][j] - go, F[i-1][j] - ge)      consumes a query letter       (CIGAR I)
    H[i][j] = max(H[i-1][j-1] + s(q[i-1], r[j-1]), E[i][j], F[i][j]),   H[0][0] = 0,   -inf off the boundary

Two statements of the same programme: `plain` is the recurrence cell by cell in Python integers, nothing else; `align` builds
each row with numpy (E along a row is a running maximum in the frame E[j] + j ge, exact because go >= ge) and keeps, per cell,
only the comparisons the walk makes.  tests/test_ends_host.py holds them against each other and against the enumeration of every
alignment; the larger GPU cases use `align`.  `rescore` knows nothing of the tie rules: it adds up what a CIGAR costs.

Sequences are arrays of codes, `mat` is n x n with mat[r][q] the score of reference code r against query code q (the matrix
hip.score_matrix and align_pairs_matrix build).  A result is the dict {score, ref_begin, ref_end, query_begin, query_end,
cigar}: coordinates 0-based and inclusive, end == begin - 1 for a span without a letter, cigar a list of (op, length), op in 'MID'."""
import random

import numpy as np

MODES = ('global', 'semiglobal', 'overlap')
NEG = -(1 << 60)


def rng_for(*key):
    return random.Random('ends/' + '/'.join(str(k) for k in key))


def dna_matrix(match, mismatch):
    """match on the diagonal, -mismatch elsewhere, 0 against N (code 4)"""
    m = np.full((5, 5), -int(mismatch), dtype=np.int64)
    np.fill_diagonal(m, int(match))
    m[4, :] = 0
    m[:, 4] = 0
    return m


def encode(seq, alphabet='ACGTN'):
    return np.array([alphabet.index(c) for c in seq], dtype=np.int64)


def _gap(k, go, ge):
    return go + (k - 1) * ge


def _boundary(mode, m, n, go, ge):
    """row 0 (n + 1 values) and column 0 (m + 1 values) of H"""
    row0 = [0] + [-_gap(j, go, ge) if mode == 'global' else 0 for j in range(1, n + 1)]
    col0 = [0] + [0 if mode == 'overlap' else -_gap(i, go, ge) for i in range(1, m + 1)]
    return row0, col0


def _end_cell(mode, m, n, last_row, last_col):
    """(i, j) of the end cell.  last_row = H[m][0..n], last_col = H[0..m][n]"""
    if mode == 'global':
        return m, n
    best, cell = None, None
    for j in range(n + 1):
        if best is None or last_row[j] > best:
            best, cell = last_row[j], (m, j)
    if mode == 'overlap':
        for i in range(m):
            if last_col[i] > best:
                best, cell = last_col[i], (i, n)
    return cell


def _walk(mode, end, diag_ok, e_ok, f_ok, e_open, f_open):
    """the walk of the definition; the five arguments answer its comparisons at a cell (i, j), i, j >= 1"""
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
        if state == 'H':
            if mode == 'global':
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
            if diag_ok(i, j):
                emit('M'); i -= 1; j -= 1
            elif e_ok(i, j):
                state = 'E'
            else:
                assert f_ok(i, j), (i, j)
                state = 'F'
        elif state == 'E':
            emit('D')
            if e_open(i, j):
                state = 'H'
            j -= 1
        else:
            emit('I')
            if f_open(i, j):
                state = 'H'
            i -= 1
    return i, j, [(o, k) for o, k in reversed(ops)]


def _result(score, end, begin, ops):
    return {'score': int(score), 'ref_begin': begin[1], 'ref_end': end[1] - 1, 'query_begin': begin[0], 'query_end': end[0] - 1, 'cigar': ops}


def plain(q, r, mat, go, ge, mode):
    """the recurrence, one cell after the other, in Python integers"""
    assert mode in MODES and go >= ge >= 0
    m, n = len(q), len(r)
    H = [[NEG] * (n + 1) for _ in range(m + 1)]
    E = [[NEG] * (n + 1) for _ in range(m + 1)]
    F = [[NEG] * (n + 1) for _ in range(m + 1)]
    row0, col0 = _boundary(mode, m, n, go, ge)
    for j in range(n + 1):
        H[0][j] = row0[j]
        if mode == 'global' and j:
            E[0][j] = row0[j]
    for i in range(1, m + 1):
        H[i][0] = col0[i]
        if mode != 'overlap':
            F[i][0] = col0[i]
    for i in range(1, m + 1):
        for j in range(1, n + 1):
            E[i][j] = max(H[i][j - 1] - go, E[i][j - 1] - ge)
            F[i][j] = max(H[i - 1][j] - go, F[i - 1][j] - ge)
            H[i][j] = max(H[i - 1][j - 1] + int(mat[r[j - 1]][q[i - 1]]), E[i][j], F[i][j])
    end = _end_cell(mode, m, n, H[m], [H[i][n] for i in range(m + 1)])
    i0, j0, ops = _walk(mode, end,
                        lambda i, j: H[i][j] == H[i - 1][j - 1] + int(mat[r[j - 1]][q[i - 1]]),
                        lambda i, j: H[i][j] == E[i][j], lambda i, j: H[i][j] == F[i][j],
                        lambda i, j: E[i][j] == H[i][j - 1] - go, lambda i, j: F[i][j] == H[i - 1][j] - go)
    return _result(H[end[0]][end[1]], end, (i0, j0), ops)


def align(q, r, mat, go, ge, mode, path=True, lines=None):
    """the same programme row by row in numpy int64; path=False: score and end cell only (begins and cigar None); `lines`, a dict,
    receives what the end cell was chosen from (last_row_and_column)"""
    assert mode in MODES and go >= ge >= 0
    q = np.asarray(q, dtype=np.int64); r = np.asarray(r, dtype=np.int64)
    mat = np.asarray(mat, dtype=np.int64)
    m, n = len(q), len(r)
    row0, col0 = _boundary(mode, m, n, go, ge)
    ar = np.arange(n + 1, dtype=np.int64) * ge
    Hp = np.array(row0, dtype=np.int64)
    Fp = np.full(n + 1, NEG, dtype=np.int64)
    flags = np.zeros((m + 1, n + 1), dtype=np.uint8) if path else None      # 1 diagonal, 2 E, 4 F reach H; 8 E opened here, 16 F opened here
    last_col = [int(Hp[n])]
    for i in range(1, m + 1):
        F = np.maximum(Hp - go, Fp - ge)
        T = np.empty(n + 1, dtype=np.int64)
        T[0] = col0[i]
        d = Hp[:-1] + mat[r, q[i - 1]] if n else np.zeros(0, dtype=np.int64)
        T[1:] = np.maximum(d, F[1:])
        E = np.full(n + 1, NEG, dtype=np.int64)
        if n:
            # E[j] = max over j' < j of H[j'] - go - (j - 1 - j') ge, and H[j'] may be replaced by T[j'] = max(diagonal, F) since go >= ge
            E[1:] = np.maximum.accumulate(T[:-1] - go + ar[1:]) - ar[1:]
        H = np.maximum(T, E)
        H[0] = col0[i]
        if path and n:
            f = (H[1:] == d).astype(np.uint8) | ((H[1:] == E[1:]).astype(np.uint8) << 1) | ((H[1:] == F[1:]).astype(np.uint8) << 2)
            f |= ((E[1:] == H[:-1] - go).astype(np.uint8) << 3) | ((F[1:] == Hp[1:] - go).astype(np.uint8) << 4)
            flags[i, 1:] = f
        Hp, Fp = H, F
        if mode != 'overlap':
            Fp[0] = col0[i]
        else:
            Fp[0] = NEG
        last_col.append(int(Hp[n]))
    end = _end_cell(mode, m, n, [int(x) for x in Hp], last_col)
    if lines is not None:
        lines.update(last_row=[int(x) for x in Hp], last_col=list(last_col))
    score = int(Hp[end[1]]) if end[0] == m else last_col[end[0]]
    if not path:
        return {'score': score, 'ref_begin': None, 'ref_end': end[1] - 1, 'query_begin': None, 'query_end': end[0] - 1, 'cigar': None}
    i0, j0, ops = _walk(mode, end, lambda i, j: flags[i, j] & 1, lambda i, j: flags[i, j] & 2, lambda i, j: flags[i, j] & 4,
                        lambda i, j: flags[i, j] & 8, lambda i, j: flags[i, j] & 16)
    return _result(score, end, (i0, j0), ops)


def last_row_and_column(q, r, mat, go, ge, mode):
    """-> (H[m][0..n], H[0..m][n]) of the programme `align` runs"""
    lines = {}
    align(q, r, mat, go, ge, mode, path=False, lines=lines)
    return lines['last_row'], lines['last_col']


def rescore(cigar, q, r, ref_begin, query_begin, mat, go, ge):
    """what a CIGAR costs, read from left to right with no knowledge of how it was chosen -> (score, reference letters, query letters)"""
    i, j, score = query_begin, ref_begin, 0
    for op, k in cigar:
        assert k > 0
        if op == 'M':
            for _ in range(k):
                score += int(mat[r[j]][q[i]]); i += 1; j += 1
        elif op == 'I':
            score -= go + (k - 1) * ge; i += k
        else:
            assert op == 'D', op
            score -= go + (k - 1) * ge; j += k
    return score, j - ref_begin, i - query_begin


def check_cigar(res, q, r, mat, go, ge, mode):
    """the CIGAR of a result rescores to its score and spans exactly its coordinates; the spans are what the mode allows"""
    m, n = len(q), len(r)
    score, nr, nq = rescore(res['cigar'], q, r, res['ref_begin'], res['query_begin'], mat, go, ge)
    assert score == res['score'], (score, res)
    assert res['ref_begin'] + nr - 1 == res['ref_end'] and res['query_begin'] + nq - 1 == res['query_end'], (nr, nq, res)
    assert 0 <= res['ref_begin'] <= res['ref_end'] + 1 <= n and 0 <= res['query_begin'] <= res['query_end'] + 1 <= m, res
    ops = [o for o, _ in res['cigar']]
    assert all(a != b for a, b in zip(ops, ops[1:])), res['cigar']
    if mode == 'global':
        assert (res['ref_begin'], res['ref_end'], res['query_begin'], res['query_end']) == (0, n - 1, 0, m - 1)
    elif mode == 'semiglobal':
        assert (res['query_begin'], res['query_end']) == (0, m - 1)
    else:
        assert res['ref_begin'] == 0 or res['query_begin'] == 0
        assert res['ref_end'] == n - 1 or res['query_end'] == m - 1


def cigar_text(ops):
    return ''.join('%d%s' % (k, o) for o, k in ops)


def parse_cigar(text):
    out, num = [], ''
    for ch in text or '':
        if ch.isdigit():
            num += ch
        else:
            out.append((ch, int(num))); num = ''
    return out


def as_tuple(res):
    return (res['score'], res['ref_begin'], res['ref_end'], res['query_begin'], res['query_end'], cigar_text(res['cigar']))


def random_seq(rng, n, alphabet='ACGT'):
    return ''.join(rng.choice(alphabet) for _ in range(n))


def mutate(rng, seq, rate, alphabet='ACGT'):
    """substitutions, insertions and deletions, each at rate / 3 per letter"""
    out = []
    for c in seq:
        x = rng.random()
        if x < rate / 3:
            out.append(rng.choice(alphabet))
        elif x < 2 * rate / 3:
            out.append(c); out.append(rng.choice(alphabet))
        elif x < rate:
            pass
        else:
            out.append(c)
    return ''.join(out)
