"""Deterministic inputs for K3 (partial-order consensus, csrc/ccs_poa.hip) through poa_batch, each built for one named edge of the
kernel (not a test module): the register counts and passes of a row, where a source row is read from (registers, the LDS ring, the
planes), in-edges in place and in the overflow table, edge weights around 255, the graph sizes at which the sort and the consensus
scores leave LDS, the longest packed sequence, ties of the best cell over register halves, lanes, passes and rows, and walks across
the back-track's staging, result ring and band.

Every position comes from constants parsed out of ccs_poa.hip (`constants()`), so the sets follow a change of POA_MAXCP or of the
LDS size; a constant that cannot be parsed raises.  Expected values are oracle/poa_oracle.c; tests/test_poa_edges_host.py proves from
the oracle's shape record (oracle_lib.oracle_poa_shape) that every case reaches what it is named for, tests/test_gpu_poa_edges.py
holds the kernel to the cases.

A case is Case(seqs, algorithm, scores, min_coverage, what): `seqs` are str whose letters are raw bytes (latin-1), `what` is a dict
that names the edge the case is built for (read by the host proofs).  Letters that occur nowhere else ("private" letters, bytes
0x80..0xff) make placements provable: a stretch written in letters of its own can only align to itself."""
import collections
import os
import random
import re

REF = (10, -4, -8, -2, -24, -1)          # the scores of every call site of the reference
CONVEX = (5, -4, -8, -6, -10, -4)        # pyspoa's defaults: two gap pieces that both matter
NOT_SIMPLE = (10, 0, -8, -2, -24, -1)    # a mismatch that costs nothing: dp_rows takes its SIMPLE pass only when every cost is negative

Case = collections.namedtuple('Case', 'seqs algorithm scores min_coverage what')

SOURCE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'ciri_long_amd', 'csrc', 'ccs_poa.hip')
PRIVATE = ''.join(chr(c) for c in range(0x80, 0x100))     # 128 letters no flank holds

_PARSED = ('POA_MAXCP', 'POA_LDS_KB', 'POA_MAXP', 'POA_MAXP_ALL', 'POA_OVF_CAP', 'POA_MAXA', 'POA_MAX_COPY', 'POA_BAND_W', 'BT_RING')
_DERIVED = ('POA_LDS_BYTES', 'POA_LDS_SCORES', 'POA_SORT_LDS', 'BT_W', 'BT_DRIFT', 'POA_BAND')


def _c_int_expr(text, names):
    """value of a C integer expression over `names`: + - * / ( ) comparisons and one ?: (the forms ccs_poa.hip uses)"""
    if not re.fullmatch(r'[\w\s+\-*/()<>=?:]+', text):
        raise ValueError('poa_edges: cannot read the expression %r' % text)
    m = re.fullmatch(r'([^?]+)\?([^:]+):(.+)', text)
    if m:
        return _c_int_expr(m.group(2) if _c_int_expr(m.group(1), names) else m.group(3), names)
    return int(eval(text.replace('/', '//'), {'__builtins__': {}}, dict(names)))


def constants(path=SOURCE):
    """the kernel's limits as ccs_poa.hip states them: `#define NAME value` (the default behind its #ifndef) or
    `static constexpr int NAME = expression;` for the parsed names, the derived ones from their own expressions in the file, RING[cp]
    from the body of poa_ring.  KeyError / ValueError where a name or a form is not found."""
    with open(path) as f:
        src = f.read()
    K = {}

    def value_of(name):
        m = re.search(r'^[ \t]*#[ \t]*define[ \t]+%s[ \t]+(\d+)\b' % name, src, re.M)
        if m:
            return int(m.group(1))
        m = re.search(r'\bconstexpr int [^;]*?\b%s = ([^,;]+)[,;]' % name, src)
        if not m:
            raise KeyError('poa_edges: %s not found in %s' % (name, path))
        return _c_int_expr(m.group(1).strip(), K)
    for name in _PARSED[:2] + ('POA_LDS_BYTES',) + _PARSED[2:] + _DERIVED[1:]:
        K[name] = value_of(name)
    # poa_ring(): a power of two of rows of `row` bytes that fits the LDS block
    body = re.search(r'int poa_ring\(int m\) \{(.*?)\n\}', src, re.S)
    row = body and re.search(r'const int row = (\d+) \* poa_ring_cp\(m\) \+ (\d+);', body.group(1))
    start = body and re.search(r'int ring = (\d+);', body.group(1))
    if not (row and start and 'while (ring * row > POA_LDS_BYTES) ring >>= 1;' in body.group(1)):
        raise ValueError('poa_edges: poa_ring() in %s no longer has the form this parser reads' % path)
    K['RING'] = {}
    for cp in range(1, K['POA_MAXCP'] + 1):
        ring = int(start.group(1))
        while ring * (int(row.group(1)) * cp + int(row.group(2))) > K['POA_LDS_BYTES']:
            ring >>= 1
        K['RING'][cp] = ring
    K['C'] = 128                               # columns of one packed register over 64 lanes (poa_cols: (m + 127) >> 7)
    K['W'] = 128 * K['POA_MAXCP']              # columns of a full pass
    return K


def _rng(*key):
    return random.Random('poa edges ' + ' '.join(str(k) for k in key))


def dna(rng, n, letters='ACGT'):
    return ''.join(rng.choice(letters) for _ in range(n))


def other(ch):
    return 'ACGT'[('ACGT'.index(ch) + 1) % 4]


def substitute(s, positions):
    s = list(s)
    for p in positions:
        s[p] = other(s[p])
    return ''.join(s)


def cols_of(m, K):
    """registers per lane of the pass that holds column m (1-based) as its last: poa_cols"""
    return min(K['POA_MAXCP'], max(1, (m + 127) >> 7))


# ----------------------------------------------------------------------------------------------------------------------------
# pass widths: 1, 2 .. POA_MAXCP registers per lane, full passes, a last pass of one column
# ----------------------------------------------------------------------------------------------------------------------------
PASS_MODES = ((0, REF), (0, NOT_SIMPLE), (1, REF), (2, REF), (1, CONVEX))


def pass_lengths(K):
    C, W = K['C'], K['W']
    return sorted({C - 1, C, C + 1, 2 * C - 1, 2 * C, 2 * C + 1, W - 1, W, W + 1, W + C, W + C + 1, 2 * W, 2 * W + 1})


def pass_family(L, K):
    """template of L letters; the same with a substitution in the first and last column of every pass (the last one the last column);
    one with an insertion in the middle, so that its last column is L + 1; a partial copy"""
    W = K['W']
    rng = _rng('pass widths', L)
    t = dna(rng, L)
    edges = sorted({p for p in list(range(0, L, W)) + list(range(W - 1, L, W)) + [L - 1]})
    return [t, substitute(t, edges), t[:L // 2] + PRIVATE[0] + t[L // 2:], t[:2 * L // 3]]


def pass_widths(K):
    return [Case(pass_family(L, K), mode, scores, 0, {'length': L}) for mode, scores in PASS_MODES for L in pass_lengths(K)]


# ----------------------------------------------------------------------------------------------------------------------------
# source distance: the row before (registers), 2 .. RING - 1 (LDS ring), >= RING (planes, every cell stored despite the band)
# ----------------------------------------------------------------------------------------------------------------------------
SOURCE_MODES = ((0, REF), (1, REF), (2, REF))


def source_distances(K):
    """[(registers per lane, template length, rank distance)]"""
    out = []
    for cp in range(1, K['POA_MAXCP'] + 1):
        ring = K['RING'][cp]
        for dist in sorted({2, ring - 1, ring, ring + 1}):
            out.append((cp, 128 * cp - 28, dist))
    out.append((K['POA_MAXCP'], 128 * K['POA_MAXCP'] - 28, 2 * K['POA_BAND'] + 9))       # the source row lies outside the target row's band
    return out


def source_family(L, dist, form):
    """deletion: the second sequence leaves out dist - 1 template letters, so the node behind them gains a predecessor dist ranks
    back; the third takes the same edge (its pass reads the far source), the fourth does not.  insertion: dist - 1 private letters
    between two template bases -- a chain whose ranks lie between theirs, so the template edge spans dist ranks.  (This second form
    stands where a substitution bubble of dist - 1 letters might: a bubble of mismatches is fused as aligned pairs, which share a
    column and leave every edge around it 2 ranks long whatever its length, and a long one is cheaper as a gap anyway -- it would
    not plant the named distance.  The inserted chain does interleave ranks, which is what the bubble was wanted for: the far edge
    belongs to the template and the ranks between its ends to another sequence.)"""
    rng = _rng('source distance', L, dist)
    t = dna(rng, L)
    a = L // 2
    if form == 'deletion':
        t = t[:a] + PRIVATE[:dist - 1] + t[a + dist - 1:]          # (private letters: no base of the gap can be matched on the way)
        s = t[:a] + t[a + dist - 1:]
        return [t, s, substitute(s, [a + 5]), substitute(t, [a - 8])]
    s = t[:a] + PRIVATE[:dist - 1] + t[a:]
    return [t, s, substitute(t, [a + 3]), substitute(s, [a - 5])]


def source_distance(K):
    return [Case(source_family(L, dist, form), mode, scores, 0, {'cp': cp, 'dist': dist, 'form': form})
            for mode, scores in SOURCE_MODES for cp, L, dist in source_distances(K) for form in ('deletion', 'insertion')]


# ----------------------------------------------------------------------------------------------------------------------------
# in-edges: 3 inline, POA_MAXP in place, the overflow table, the 4-bit count that saturates at 15, POA_MAXP_ALL
# ----------------------------------------------------------------------------------------------------------------------------
FLANK = 12
IN_EDGE_MODES = SOURCE_MODES


def in_edge_repeats(degree):
    """sequences that enter through the last predecessor added: the first creates the edge, two raise its weight -- and as many more
    as the consensus needs to run through that edge and not through the motif: the heaviest bundle ends in the node with the largest
    sum of weights, the motif's edges sum to (degree - 1)(degree - 2) (2 per sequence that holds them), the flank behind the
    junction to 2 (FLANK - 1) per sequence plus 2 per repeat"""
    motif = (degree - 1) * (degree - 2)
    r = 3
    while 2 * r + 2 * (FLANK - 1) * (degree - 1 + r) <= motif + 2 * FLANK * degree:
        r += 1
    return r


def in_degrees(K):
    return sorted({3, 4, K['POA_MAXP'], K['POA_MAXP'] + 1, 14, 15, 16, K['POA_MAXP_ALL'] - 1, K['POA_MAXP_ALL']})


def junction_seqs(degrees, key):
    """one sequence per k = 0 .. max(degrees) - 1: F0 + M1[:n1 - k] + F1 + M2[:n2 - k] + F2 ..., F* flanks of FLANK random ACGT
    letters, M* motifs of n* = degree - 1 private letters (each motif distinct letters; a negative end is empty).  The first node of
    F_j gains one predecessor per distinct length of M_j: M_j's last letter, its last but one, ..., the last letter of F_{j-1}:
    in-degree = degree_j."""
    rng = _rng('junctions', key)
    flanks = [dna(rng, FLANK) for _ in range(len(degrees) + 1)]
    motifs = [''.join(PRIVATE[(17 * j + i) % len(PRIVATE)] for i in range(d - 1)) for j, d in enumerate(degrees)]
    seqs = []
    for k in range(max(degrees)):
        s = flanks[0]
        for j, mo in enumerate(motifs):
            s += mo[:max(0, len(mo) - k)] + flanks[j + 1]
        seqs.append(s)
    return seqs


def in_edge_family(degree):
    seqs = junction_seqs([degree], ('in-edges', degree))
    return seqs + [seqs[-1]] * (in_edge_repeats(degree) - 1)


def in_edges(K):
    return [Case(in_edge_family(d), mode, scores, 0, {'indeg': d}) for mode, scores in IN_EDGE_MODES for d in in_degrees(K)]


def in_edges_refused(K):
    """one in-edge more than the kernel keeps: status 2 (the oracle answers it)"""
    d = K['POA_MAXP_ALL'] + 1
    return Case(junction_seqs([d], ('in-edges', d)), 1, REF, 0, {'indeg': d})


# ----------------------------------------------------------------------------------------------------------------------------
# overflow table: entries of several nodes interleave; exactly POA_OVF_CAP entries, and one more
# ----------------------------------------------------------------------------------------------------------------------------
OVERFLOW_JUNCTIONS = 12


def overflow_total(degrees, K):
    return sum(max(0, d - K['POA_MAXP']) for d in degrees)


def overflow_interleaved(K):
    """12 junctions of in-degree POA_MAXP_ALL, POA_MAXP_ALL - 1, ... in one group: sequence k adds an entry to every junction that
    is past POA_MAXP, so the entries of different nodes alternate in the table"""
    degrees = [K['POA_MAXP_ALL'] - (j % 5) for j in range(OVERFLOW_JUNCTIONS)]
    return [Case(junction_seqs(degrees, 'overflow interleaved'), mode, scores, 0, {'degrees': degrees})
            for mode, scores in IN_EDGE_MODES]


def overflow_capacity_degrees(K, extra=0):
    """junction in-degrees whose overflow entries total POA_OVF_CAP + extra: as many junctions of in-degree POA_MAXP_ALL as fit, one
    for the rest"""
    per = K['POA_MAXP_ALL'] - K['POA_MAXP']
    full, rest = divmod(K['POA_OVF_CAP'] + extra, per)
    return [K['POA_MAXP_ALL']] * full + ([K['POA_MAXP'] + rest] if rest else [])


def overflow_capacity(K, extra=0):
    """sequences above POA_MAX_COPY letters: the wide form of the pass"""
    degrees = overflow_capacity_degrees(K, extra)
    return Case(junction_seqs(degrees, 'overflow capacity'), 1, REF, 0, {'degrees': degrees, 'total': K['POA_OVF_CAP'] + extra})


# ----------------------------------------------------------------------------------------------------------------------------
# weights: the heaviest-bundle pass takes rows with an in-edge weight above 255 by another path
# ----------------------------------------------------------------------------------------------------------------------------
WEIGHT_COUNTS = (127, 128, 129)          # identical sequences: edge weights 254, 256, 258
SCORE_COUNTS = (64, 65, 66)              # the API returns the end-cell scores of the first 65 sequences
WEIGHT_MODES = ((1, REF), (0, REF))


def weight_family(n, minority=3):
    """n identical sequences of 30 letters and `minority` that differ in letters 14..16 (a branch the bundle must not take); the
    minority come second, fourth, ..., so the branch exists while the weights grow"""
    rng = _rng('weights')
    t = dna(rng, 30)
    alt = t[:14] + PRIVATE[:3] + t[17:]
    seqs = [t] * n
    for k in range(minority):
        seqs.insert(1 + 2 * k, alt)
    return seqs


def weights(K):
    out = []
    for mode, scores in WEIGHT_MODES:
        for n in WEIGHT_COUNTS:
            seqs = weight_family(n)
            for mc in (0, (len(seqs) + 1) // 2):
                out.append(Case(seqs, mode, scores, mc, {'weight': 2 * n}))
    return out


def score_counts(K):
    return [Case(weight_family(n - 3), 1, REF, 0, {'count': n}) for n in SCORE_COUNTS]


# ----------------------------------------------------------------------------------------------------------------------------
# graph size: the sort leaves LDS above POA_SORT_LDS nodes, the consensus scores above POA_LDS_SCORES rows, the packed form of the
# pass ends at POA_MAX_COPY letters
# ----------------------------------------------------------------------------------------------------------------------------
SIZE_MODES = ((1, REF), (0, REF))


def node_counts(K):
    return [K['POA_SORT_LDS'] + d for d in (-1, 0, 1)] + [K['POA_LDS_SCORES'] + d for d in (-1, 0, 1)]


def size_family(nodes, key='graph size'):
    """two sequences whose graph has exactly `nodes` nodes: a template of nodes - s letters and the same with s substitutions, each
    of which adds one node (s = 10 + nodes % 7)"""
    s = 10 + nodes % 7
    L = nodes - s
    rng = _rng(key, nodes)
    t = dna(rng, L)
    step = L // (s + 1)
    return [t, substitute(t, [step * (k + 1) for k in range(s)])]


def copy_lengths(K):
    return [K['POA_MAX_COPY'] + d for d in (-1, 0, 1)]


def copy_family(L):
    rng = _rng('copy length', L)
    t = dna(rng, L)
    return [t, substitute(t, [7, L // 2, L - 9]), t[:L // 2 - 1] + t[L // 2:]]


def graph_size(K):
    out = [Case(size_family(n), mode, scores, 0, {'nodes': n}) for mode, scores in SIZE_MODES for n in node_counts(K)]
    out += [Case(copy_family(L), mode, scores, 0, {'length': L}) for mode, scores in SIZE_MODES for L in copy_lengths(K)]
    return out


# ----------------------------------------------------------------------------------------------------------------------------
# ties: spoa takes the smallest row, then the smallest column; the kernel reduces over register halves, lanes, passes
# ----------------------------------------------------------------------------------------------------------------------------
def column_tie(first, second, total, u_len=1):
    """local mode.  The graph is X + U + Y (ACGT, U in private letters); the sequence holds U at columns `first` and `second`
    (1-based column of U's last letter) between private letters the graph does not have: the same score in the same row at two
    columns.  -> (seqs, the sequence with only the second U: the proof that the second cell scores the same)"""
    rng = _rng('ties', first, second, total)
    u = PRIVATE[100:100 + u_len]
    graph = dna(rng, 7) + u + dna(rng, 7)
    fill = [PRIVATE[(3 * i) % 90] for i in range(total)]
    only_second = list(fill)
    for end in (first, second):
        fill[end - u_len:end] = u
    only_second[second - u_len:second] = u
    assert len(fill) == total and first + u_len <= second
    return [graph, ''.join(fill)], [graph, ''.join(only_second)]


ROW_TIE_U = PRIVATE[100:105]


def tie_cases(K):
    """-> [(Case, seqs of the proof, what)]"""
    C, W = K['C'], K['W']
    out = []
    for cp in range(1, K['POA_MAXCP'] + 1):          # lane l owns columns 2 cp l .. 2 cp l + 2 cp - 1; register t holds columns t and cp + t of them
        total = 128 * cp - 9
        for o in range(2 * cp):
            first = 2 * cp * 11 + o + 1
            seqs, proof = column_tie(first, first + cp, total)
            out.append((Case(seqs, 0, REF, 0, {'tie': 'halves' if o < cp else 'neighbours', 'cp': cp, 'columns': (first, first + cp)}), proof))
        seqs, proof = column_tie(2 * cp * 5 + 3, 2 * cp * 40 + 2, total, u_len=4)
        out.append((Case(seqs, 0, REF, 0, {'tie': 'lanes', 'cp': cp, 'columns': (2 * cp * 5 + 3, 2 * cp * 40 + 2)}), proof))
    for first, second, total in ((W - 1, W + 1, W + 50), (W, W + 1, W + 50), (40, W + C + 7, W + C + 30), (W - 3, 2 * W + 5, 2 * W + 9)):
        seqs, proof = column_tie(first, second, total, u_len=1 if second - first < 8 else 5)
        out.append((Case(seqs, 0, REF, 0, {'tie': 'passes', 'columns': (first, second)}), proof))
    for total in (40, C + 30, W + 30):                # two rows in one column: the graph is U + X + U, the sequence holds U once
        rng = _rng('row tie', total)
        u = ROW_TIE_U
        x = dna(rng, 9)
        fill = [PRIVATE[(3 * i) % 90] for i in range(total)]
        fill[total - 20:total - 15] = u
        seq = ''.join(fill)
        out.append((Case([u + x + u, seq], 0, REF, 0, {'tie': 'rows', 'column': total - 15}), [PRIVATE[110:115] + x + u, seq]))
    return out


def ties(K):
    return [c for c, _ in tie_cases(K)]


# ----------------------------------------------------------------------------------------------------------------------------
# walks: horizontal runs across the staged band's width and drift and across the result ring; vertical runs across the re-stage
# after 48 rows; a leading insertion swept across the band of stored cells
# ----------------------------------------------------------------------------------------------------------------------------
WALK_FLANK = 40
WALK_DELETIONS = (47, 48, 49, 64, 65)
WALK_MODES = ((1, REF), (2, REF), (0, REF))


def walk_insertions(K):
    h = K['BT_RING'] // 2
    return sorted({K['BT_DRIFT'] - 1, K['BT_DRIFT'], K['BT_W'], 64, h - 1, h, h + 1, K['BT_RING'], K['BT_RING'] + 1})


def gap_cost(k):
    g, e, q, c = REF[2:]
    return -max(g + (k - 1) * e, q + (k - 1) * c)


def walk_flank(k, mode):
    """40 letters; in local and overlap mode (the sequence's end is free there) both flanks stay in the alignment only while a flank
    scores more than the gap between them costs, so the long runs get flanks that do"""
    return WALK_FLANK if mode == 1 else max(WALK_FLANK, gap_cost(k) // REF[0] + 2)


def insertion_walk(k, mode=1):
    """flank + flank, then the same around k private letters (a horizontal run of k), then the first again"""
    rng = _rng('walks insertion')
    n = walk_flank(k, mode)
    a, b = dna(rng, n), dna(rng, n)
    return [a + b, a + ''.join(PRIVATE[i % len(PRIVATE)] for i in range(k)) + b, a + b]


def deletion_walk(d):
    """flank + d letters + flank, then the flanks alone (a vertical run of d), then the first again"""
    rng = _rng('walks deletion')
    a, b = dna(rng, WALK_FLANK), dna(rng, WALK_FLANK)
    return [a + PRIVATE[:d] + b, a + b, a + PRIVATE[:d] + b]


def walks(K):
    out = []
    for mode, scores in WALK_MODES:
        out += [Case(insertion_walk(k, mode), mode, scores, 0, {'hrun': k}) for k in walk_insertions(K)]
        out += [Case(deletion_walk(d), mode, scores, 0, {'vrun': d}) for d in WALK_DELETIONS]
    return out


BAND_MODES = ((0, REF), (1, REF))


def band_steps(K):
    return list(range(K['POA_BAND'] - 8, K['POA_BAND'] + 9, 2))


def band_sweep(K):
    """a template of 300 letters, three sequences in the graph, then the template behind k private letters"""
    rng = _rng('walks band')
    t = dna(rng, 300)
    graph = [t, substitute(t, [50, 150]), substitute(t, [100, 250])]
    return [Case(graph + [PRIVATE[:k] + t], mode, scores, 0, {'lead': k}) for mode, scores in BAND_MODES for k in band_steps(K)]


# ----------------------------------------------------------------------------------------------------------------------------
# tandem reads: the same pass edges entering K3 from K2 (find_consensus)
# ----------------------------------------------------------------------------------------------------------------------------
TANDEM_COPIES = 8


def tandem_periods(K):
    C, W = K['C'], K['W']
    return [C, C + 1, W, W + 1, W + C, W + C + 1]


def tandem_reads(K):
    """exact tandem reads (no mutation): 8 copies of a random unit of each period"""
    return [dna(_rng('tandem', p), p) * TANDEM_COPIES for p in tandem_periods(K)]


SETS = collections.OrderedDict([
    ('pass widths', pass_widths), ('source distance', source_distance), ('in-edges', in_edges), ('overflow table', overflow_interleaved),
    ('weights', weights), ('score counts', score_counts), ('graph size', graph_size), ('ties', ties), ('walks', walks),
    ('band sweep', band_sweep),
])


def batches(cases):
    """cases that share mode, scores and min_coverage go to the device as groups of one call: -> [((algorithm, scores, min_coverage), [cases])]"""
    out = collections.OrderedDict()
    for c in cases:
        out.setdefault((c.algorithm, c.scores, c.min_coverage), []).append(c)
    return list(out.items())
