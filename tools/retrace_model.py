"""K1g's recompute route to the CIGARs (csrc/ssw_ends.hip, pr_walk_round in csrc/ssw_pairs.h) in Python, for any chunk width: the scheme,
not the definition (those are tests/ends_check.py, anchored_check.py, twopiece_check.py and spliced_check.py).

A chunk is cpl * lanes reference columns.  The row step of a chunk is that of tools/ends_model.py, twopiece_model.py and
spliced_model.py, written here cell by cell (the lanes' scans are exact, so a cell's values and decision bits are the same): what the
scheme adds does not look inside it.  Three passes:

  keep    the score pass, chunk after chunk over all rows, every chunk but the last leaving its last column -- NH values per row: H, E
          (one piece), H, E_1, E_2 (two pieces), T, E, N (spliced) -- in a slot of its own; chunk c reads slot c - 1, chunk 0 the
          mode's column 0.  It leaves the score, the end cell and the walk's fresh record: the end cell, its chunk, state 0, no open
          run, i + j + 2 steps.
  tile    the storing row step over the one chunk c and the rows 1..i the record names, its incoming column from slot c - 1: the
          decisions of those cells, the same bits the stored route leaves.
  walk    the walk of the stored route over that tile.  When the next cell lies left of the tile (0 < j <= c0) it saves (i, j, state,
          the open run, the ops so far, the steps left), names chunk c - 1 and returns: the next round's tile is that chunk.  An E or
          N run of the spliced walk is taken up to cpl cells at a step out of one stored word and so ends at the tile's edge too.

The column only decreases, so a pair moves one chunk back per round and is done within nchunks rounds; a run that crosses a chunk edge
comes out as one op because the open run is in the record; the budget of i + j + 2 steps is spent once.  `stats`, a dict, receives
the rounds, the cells computed a second time and the steps left at the end.

model: 'one' with costs (go, ge); 'two' with (go1, ge1, go2, ge2); 'spliced' with spliced_check.make_costs(...) and a strand.

`fault` plants one wrong line (tests/test_retrace_host.py names the case set that catches each):
    'slot_c'        the tile reads kept slot c, not c - 1        'limit_short'   the tile's row limit one short
    'run_dropped'   the open run flushed at a suspend            'budget_renew'  i + j + 2 steps anew every round
    'state_t_lost'  spliced: state T saved as state 0            'run_past_edge' run_left goes on past the tile's left edge
    'chunk0_kept'   chunk 0 reads kept slot 0, not column 0"""
MODES = ('global', 'semiglobal', 'overlap', 'prefix', 'extend')
ANCHORED = ('global', 'prefix', 'extend')
MODELS = ('one', 'two', 'spliced')
FAULTS = ('slot_c', 'limit_short', 'run_dropped', 'budget_renew', 'state_t_lost', 'run_past_edge', 'chunk0_kept')
OTHER = 64
NO_WALK = 'no walk'          # EN_ST_NO_WALK: what does not add up is refused, never returned


class _Pair(object):
    """one pair under one model: boundary values, the incoming column of chunk 0, and the row step of one cell"""

    def __init__(self, model, q, r, mat, costs, mode, strand):
        self.model, self.q, self.r, self.mat, self.mode = model, q, r, mat, mode
        self.m, self.n = len(q), len(r)
        if model == 'one':
            self.go, self.ge = costs
            assert self.go >= self.ge >= 0
        elif model == 'two':
            self.go, self.ge, self.go2, self.ge2 = costs
            assert 0 <= self.ge2 <= self.ge <= self.go <= self.go2
        else:
            self.go, self.ge, self.io = costs[:3]
            donor, acceptor, other = costs[3:]
            site = [0] * 65
            for x in range(4):
                for y in range(4):
                    site[4 * x + y] = donor[4 * x + y]; site[16 + 4 * x + y] = acceptor[4 * x + y]
                    site[32 + 4 * x + y] = acceptor[4 * (3 - y) + (3 - x)]; site[48 + 4 * x + y] = donor[4 * (3 - y) + (3 - x)]
            site[OTHER] = other
            self.site, self.soff = site, (32 if strand < 0 else 0)

    def letter(self, pos):
        return int(self.r[pos]) if 0 <= pos < self.n else 4

    def cost(self, which, x, y):
        return self.site[OTHER if (x | y) > 3 else self.soff + which + 4 * x + y]

    def iod(self, j):
        """io + don(j + 1): what opening an intron behind the 1-based column j costs"""
        return self.io + self.cost(0, self.letter(j), self.letter(j + 1))

    def acc(self, j):
        return self.cost(16, self.letter(j - 2), self.letter(j - 1))

    def gap(self, k):
        a = self.go + (k - 1) * self.ge
        return min(a, self.go2 + (k - 1) * self.ge2) if self.model == 'two' else a

    def row0(self, j):
        if self.mode not in ANCHORED or j == 0:
            return 0
        if self.model == 'spliced':
            return -min(self.go + (j - 1) * self.ge, self.iod(0) + self.acc(j))
        return -self.gap(j)

    def col0(self, i):
        return 0 if (self.mode == 'overlap' or i == 0) else -self.gap(i)

    def row0_op(self, j):
        if self.model != 'spliced':
            return 'D'
        return 'D' if self.go + (j - 1) * self.ge <= self.iod(0) + self.acc(j) else 'N'

    def column0(self, i):
        """what chunk 0 takes for the column in front of it, row i: the NH values, E (and E_2, N) one opening below H"""
        h = self.col0(i)
        if self.model == 'one':
            return (h, h - self.go)
        if self.model == 'two':
            return (h, h - self.go, h - self.go2)
        return (h, None, None)          # spliced: E0 = T - go and N0 = T - iod_in alone

    def chunk(self, c0, cols, ilim, incoming, cells=None, heights=None):
        """rows 1..ilim of the chunk of columns c0 + 1 .. c0 + cols; incoming(i) is the kept column c0 of row i >= 1.  Fills `cells` with
        the decision bits and `heights` with H, and returns the chunk's last column, a tuple of NH values per row."""
        go, ge, model = self.go, self.ge, self.model
        out = []
        Hp = [self.row0(c0 + t) for t in range(cols + 1)]          # H[i-1][c0 ..]
        Fp = [h - go for h in Hp]
        F2p = [h - self.go2 for h in Hp] if model == 'two' else None
        for i in range(1, ilim + 1):
            vin = incoming(i)
            H = [0] * (cols + 1); F = [0] * (cols + 1); F2 = [0] * (cols + 1)
            if model == 'one':
                hin, ein = vin
                H[0] = hin
                e, tl = max(ein - ge, hin - go), None
            elif model == 'two':
                hin, e1in, e2in = vin
                H[0] = hin
                e, e2 = max(e1in - ge, hin - go), max(e2in - self.ge2, hin - self.go2)
            else:
                tin, ein, nin = vin
                if ein is None:
                    H[0], e, u = tin, tin - go, tin - self.iod(c0)
                else:
                    H[0] = max(tin, ein, nin - self.acc(c0))
                    e, u = max(ein - ge, tin - go), max(nin, tin - self.iod(c0))
                tl, xl = tin, tin - self.iod(c0)
            last = None
            for t in range(1, cols + 1):
                j = c0 + t
                s = int(self.mat[self.r[j - 1]][self.q[i - 1]])
                D = Hp[t - 1] + s
                F[t] = max(Hp[t] - go, Fp[t] - ge)
                if model == 'one':
                    T = max(D, F[t])
                    H[t] = max(T, e)
                    b = (0 if H[t] == D else (1 if H[t] == e else 2)) | (4 if e == H[t - 1] - go else 0) | (8 if F[t] == Hp[t] - go else 0)
                    last = (H[t], e)
                    e = max(e - ge, T - go)
                elif model == 'two':
                    F2[t] = max(Hp[t] - self.go2, F2p[t] - self.ge2)
                    T = max(D, F[t], F2[t])
                    H[t] = max(T, e, e2)
                    src = [D, e, e2, F[t], F2[t]].index(H[t])
                    b = src | (8 if e == H[t - 1] - go else 0) | (16 if e2 == H[t - 1] - self.go2 else 0) | \
                        (32 if F[t] == Hp[t] - go else 0) | (64 if F2[t] == Hp[t] - self.go2 else 0)
                    last = (H[t], e, e2)
                    e, e2 = max(e - ge, T - go), max(e2 - self.ge2, T - self.go2)
                else:
                    T = max(D, F[t])
                    a = self.acc(j)
                    H[t] = max(T, e, u - a)
                    src = [D, e, u - a, F[t]].index(H[t])
                    b = src | (0 if T == D else 4) | (8 if e == tl - go else 0) | (16 if u == xl else 0) | (32 if F[t] == Hp[t] - go else 0)
                    last = (T, e, u)
                    tl, xl = T, T - self.iod(j)
                    e, u = max(e - ge, T - go), max(u, xl)
                if cells is not None:
                    cells[(i, j)] = b
                if heights is not None:
                    heights[(i, j)] = H[t]
            out.append(last)
            Hp, Fp, F2p = H, F, F2
        return out


def _end_cell(pair, heights):
    m, n, mode = pair.m, pair.n, pair.mode
    if mode == 'global':
        return heights[(m, n)], (m, n)
    if mode == 'extend':
        best = (0, 0, 0)
        for i in range(1, m + 1):
            for j in range(1, n + 1):
                if heights[(i, j)] > best[0]:
                    best = (heights[(i, j)], i, j)
        return best[0], (best[1], best[2])
    row_best, row_j = pair.col0(m), 0
    for j in range(1, n + 1):
        if heights[(m, j)] > row_best:
            row_best, row_j = heights[(m, j)], j
    if mode != 'overlap':
        return row_best, (m, row_j)
    col_best, col_i = 0, 0
    for i in range(1, m):
        if heights[(i, n)] > col_best:
            col_best, col_i = heights[(i, n)], i
    return (row_best, (m, row_j)) if row_best >= col_best else (col_best, (col_i, n))


def walk_round(pair, rec, cells, c, C, cpl, last_round, fault=None):
    """pr_walk_round: one round of the walk over the tile of chunk c; -> True when the pair is done (rec['ops'] final, or rec['bad'])"""
    c0 = c * C
    spliced = pair.model == 'spliced'
    n_ref, n_gap = (1, 2) if pair.model == 'one' else ((2, 4) if pair.model == 'two' else (2, 3))
    open1 = 4 if pair.model == 'one' else 8
    src_mask = 7 if pair.model == 'two' else 3
    i, j, state, ops = rec['i'], rec['j'], rec['state'], rec['ops']
    if rec['chunk'] != c or not (c0 + 1 if c else 0) <= j <= min(pair.n, c0 + C):
        rec['bad'] = True
        return True

    def emit(op, k=1):
        if k <= 0:
            return
        if ops and ops[-1][0] == op and rec['open']:
            ops[-1][1] += k
        else:
            ops.append([op, k]); rec['open'] = True
    while rec['steps'] > 0:
        if (state == 0 or (spliced and state == 4)) and (i == 0 or j == 0):      # spliced: 4 is state T
            if pair.mode in ANCHORED:
                if j > 0:
                    emit(pair.row0_op(j), j)
                emit('I', i); i = j = 0
            elif pair.mode == 'semiglobal' and j == 0:
                emit('I', i); i = 0
            rec.update(i=i, j=j, state=state)
            return True
        if 0 < j <= c0:
            if last_round:
                break
            rec.update(chunk=c - 1, i=i, j=j, state=0 if (fault == 'state_t_lost' and state == 4) else state)
            if fault == 'run_dropped':
                rec['open'] = False
            return False
        rec['steps'] -= 1
        if (i, j) not in cells:
            break
        b = cells[(i, j)]
        if state == 0:
            state = b & src_mask
            if state == 0:
                emit('M'); i -= 1; j -= 1
                continue
        elif spliced and state == 4:
            if not b & 4:
                emit('M'); i -= 1; j -= 1; state = 0
                continue
            state = 3
        opened = (open1 >> 1) << state
        if state <= n_ref:
            if spliced:
                # run_left: the cells of the run in the word of (i, j), leftwards up to the first whose "opened here" is set
                k, done = 0, False
                while True:
                    if (i, j - k) not in cells:
                        k = -1
                        break
                    done = bool(cells[(i, j - k)] & opened)
                    k += 1
                    at_edge = (j - k - c0) % cpl == 0 if fault != 'run_past_edge' else (j - k) % (2 * C) == 0
                    if done or at_edge:
                        break
                if k <= 0:
                    break
                emit('D' if state == 1 else 'N', k); j -= k
                if done:
                    state = 4
            else:
                emit('D'); j -= 1
                if b & opened:
                    state = 0
        elif state <= n_gap:
            emit('I'); i -= 1
            if b & opened:
                state = 0
        else:
            break
    rec['bad'] = True
    return True


def run(model, q, r, mat, costs, mode, strand=1, cpl=8, lanes=64, fault=None, stats=None):
    """-> the result dict of tests/ends_check.py, or NO_WALK where the walk refuses"""
    assert model in MODELS and mode in MODES and fault in (None,) + FAULTS
    pair = _Pair(model, q, r, mat, costs, mode, strand)
    m, n = pair.m, pair.n
    assert m > 0 and n > 0, 'a pair with an empty side never reaches the kernel'
    C = cpl * lanes
    nchunks = (n + C - 1) // C
    # keep: the score pass; slot c is the last column of chunk c
    kept, heights = [], {}
    for c in range(nchunks):
        incoming = (lambda i: pair.column0(i)) if c == 0 else (lambda i, col=kept[c - 1]: col[i - 1])
        col = pair.chunk(c * C, min(C, n - c * C), m, incoming, heights=heights)
        if c < nchunks - 1:
            kept.append(col)
    score, (ei, ej) = _end_cell(pair, heights)
    rec = dict(chunk=(ej - 1) // C if ej > 0 else 0, i=ei, j=ej, state=0, ops=[], open=False, steps=ei + ej + 2, bad=False)
    rounds = recomputed = 0
    done = False
    while not done and rounds < nchunks:
        c, ilim = rec['chunk'], rec['i']
        cells = {}
        if ilim > 0 and rec['j'] > 0:
            if fault == 'limit_short':
                ilim -= 1
            if c == 0 and not (fault == 'chunk0_kept' and kept):
                incoming = lambda i: pair.column0(i)
            else:
                slot = c if (fault == 'slot_c' and c < len(kept)) else max(c - 1, 0)
                incoming = lambda i, col=kept[slot]: col[i - 1]
            pair.chunk(c * C, min(C, n - c * C), ilim, incoming, cells=cells)
            recomputed += len(cells)
        if fault == 'budget_renew':
            rec['steps'] = rec['i'] + rec['j'] + 2
        rounds += 1
        done = walk_round(pair, rec, cells, c, C, cpl, rounds == nchunks, fault)
    if stats is not None:
        stats.update(rounds=rounds, recomputed=recomputed, steps_left=rec['steps'], nchunks=nchunks)
    if rec['bad'] or not done:
        return NO_WALK
    return {'score': score, 'ref_begin': rec['j'], 'ref_end': ej - 1, 'query_begin': rec['i'], 'query_end': ei - 1,
            'cigar': [(o, k) for o, k in reversed(rec['ops'])]}
