"""The plain statement of K7j (csrc/seed_junction.hip): a back-splice junction refined to the base, and what ciri_long_amd.seed makes of
it (refine_junctions, call_circles, the pieces map_spliced(refine=True) aligns).  Written from the definition of include/ciri_long_hip.h;
the yardstick of tests/test_junction_host.py and tests/test_gpu_junction.py (not a test module).

A task is (minus, xd, yd, xa, ya, strand) on one contig (a list of codes 0..4) and one read (codes as given).  S is the read as the
strand reads it.  With m = ya - yd:  Q = S[yd:ya), D = contig[xd : min(xd + m + slack, len)), A = contig[max(0, xa - m - slack) : xa).
HL[t][u] is the global affine score of Q[0:t) against D[0:u), HR[t][v] that of Q[t:m) against the last v letters of A: equal codes
below 4 score +match, everything else -mismatch, a gap of g letters costs gap_open + (g - 1) gap_extend.  The skipped run starts at
a = xd + u and ends at b = xa - v - 1; its start and end cost come from the dinucleotides (a, a + 1) and (b - 1, b) on the strand.

    J(s, t, u, v) = HL[t][u] + HR[t][v] - start_s(xd + u) - end_s(xa - v - 1) - intron_open

The answer is the maximum; ties go to strand +, then the smallest t, then the smallest u, then the smallest v."""
import numpy as np

import seed_check as sc

DEFAULTS = dict(match=2, mismatch=2, gap_open=3, gap_extend=1, intron_open=12, noncanonical=6, donor_costs=None, acceptor_costs=None, slack=16, max_span=512)
MAX_SPAN, MAX_SLACK, BOUND = 512, 64, 1 << 20
NEG = -(1 << 60)


def parameters(p):
    unknown = set(p) - set(DEFAULTS)
    assert not unknown, unknown
    out = dict(DEFAULTS)
    out.update(p)
    return out


def tables(p):
    """-> (donor[16], acceptor[16], other): GT as donor and AG as acceptor cost 0, everything else `noncanonical`, the dicts override"""
    donor, acceptor = [p['noncanonical']] * 16, [p['noncanonical']] * 16
    donor[4 * 2 + 3] = 0
    acceptor[4 * 0 + 2] = 0
    for table, over in ((donor, p['donor_costs']), (acceptor, p['acceptor_costs'])):
        for key, v in (over or {}).items():
            table[4 * 'ACGT'.index(key[0].upper()) + 'ACGT'.index(key[1].upper())] = int(v)
    return donor, acceptor, p['noncanonical']


def admitted(p):
    """what the limits of the definition admit: None, or the code of the refusal (-2 CLH_E_ARG, -3 CLH_E_UNSUPPORTED)"""
    donor, acceptor, other = tables(p)
    costs = [p['match'], p['mismatch'], p['gap_open'], p['gap_extend'], p['intron_open'], other] + donor + acceptor
    if not 1 <= p['max_span'] <= MAX_SPAN or not 0 <= p['slack'] <= MAX_SLACK or min(costs) < 0:
        return -2
    if p['gap_open'] < p['gap_extend']:
        return -3
    if (2 * p['max_span'] + p['slack']) * max(costs[:4]) + p['intron_open'] + max(donor + [other]) + max(acceptor + [other]) >= BOUND:
        return -2
    return None


def letter(contig, x):
    return contig[x] if 0 <= x < len(contig) else 4


def site(contig, p, part, minus, tabs):
    """the cost of the dinucleotide at (p, p + 1) as the start (part 0) or the end (part 1) of a skipped run on strand + / -"""
    donor, acceptor, other = tabs
    a, b = letter(contig, p), letter(contig, p + 1)
    if a > 3 or b > 3:
        return other
    if not minus:
        return (donor, acceptor)[part][4 * a + b]
    return (acceptor, donor)[part][4 * (3 - b) + (3 - a)]


def status(xd, yd, xa, ya, max_span):
    if ya - yd > max_span:
        return 1
    if ya - yd < 1 or xa >= xd:
        return 2
    return 0


def windows(contig, xd, xa, m, slack):
    """-> (D, A reversed): the letters forward from the donor anchor and those backwards from the acceptor anchor"""
    return contig[xd:min(xd + m + slack, len(contig))], contig[max(0, xa - m - slack):xa][::-1]


def side(q, r, p):
    """H[t][u] of q[0:t) against r[0:u), global: every row built with numpy from the row above (the gap along a row is a running maximum
    in the frame E[u] + u ge, exact because gap_open >= gap_extend); tests/test_junction_host.py holds it to ends_check.plain"""
    go, ge = p['gap_open'], p['gap_extend']
    q, r = np.asarray(q, dtype=np.int64), np.asarray(r, dtype=np.int64)
    m, n = len(q), len(r)
    H = np.zeros((m + 1, n + 1), dtype=np.int64)
    ar = np.arange(n + 1, dtype=np.int64) * ge
    H[0, 1:] = -(go + ar[:n])
    F = np.full(n + 1, NEG, dtype=np.int64)
    for t in range(1, m + 1):
        F = np.maximum(H[t - 1] - go, F - ge)
        T = np.empty(n + 1, dtype=np.int64)
        T[0] = -(go + (t - 1) * ge)
        if n:
            s = np.where((r == q[t - 1]) & (r < 4), p['match'], -p['mismatch'])
            T[1:] = np.maximum(H[t - 1, :-1] + s, F[1:])
            E = np.maximum.accumulate(T[:-1] - go + ar[1:]) - ar[1:]
            H[t, 1:] = np.maximum(T[1:], E)
        H[t, 0] = T[0]
        F[0] = NEG
    return H


def sides(contig, read, task, p):
    """-> (HL, HR[t][v], start[s][u], end[s][v]) of a task of status 0"""
    minus, xd, yd, xa, ya, _ = task
    S = sc.revcomp(read) if minus else list(read)
    m = ya - yd
    Q = S[yd:ya]
    D, Ar = windows(contig, xd, xa, m, p['slack'])
    HL = side(Q, D, p)
    HR = side(Q[::-1], Ar, p)[::-1]                     # row m - t of the reversed problem is Q[t:m)
    tabs = tables(p)
    start = [np.array([site(contig, xd + u, 0, s, tabs) for u in range(len(D) + 1)], dtype=np.int64) for s in (0, 1)]
    end = [np.array([site(contig, xa - v - 2, 1, s, tabs) for v in range(len(Ar) + 1)], dtype=np.int64) for s in (0, 1)]
    return HL, HR, start, end


def refine(contig, read, task, **p):
    """the row of a task as the kernel writes it: [status, score, strand, t, u, v, donor_end, acceptor_start, HL, HR, start cost, end cost]"""
    p = parameters(p)
    assert admitted(p) is None
    minus, xd, yd, xa, ya, strand = task
    st = status(xd, yd, xa, ya, p['max_span'])
    if st:
        return [st] + [0] * 11
    HL, HR, start, end = sides(contig, read, task, p)
    best = None
    for s in (0, 1):
        if strand == (-1, 1)[s]:
            continue
        L, R = HL - start[s][None, :], HR - end[s][None, :]
        for t in range(ya - yd + 1):
            u, v = int(np.argmax(L[t])), int(np.argmax(R[t]))          # the first of the greatest: the smallest index
            J = int(L[t, u] + R[t, v]) - p['intron_open']
            if best is None or J > best[0]:
                best = (J, s, t, u, v)
    J, s, t, u, v = best
    return [0, J, s, t, u, v, xd + u, xa - v, int(HL[t, u]), int(HR[t, v]), int(start[s][u]), int(end[s][v])]


def maxima(contig, read, task, **p):
    """every (s, t) at which the maximum of J is reached, for the tie tests: [(s, t)]"""
    p = parameters(p)
    HL, HR, start, end = sides(contig, read, task, p)
    got = {}
    for s in (0, 1):
        if task[5] != (-1, 1)[s]:
            for t in range(task[4] - task[2] + 1):
                got[(s, t)] = int((HL[t] - start[s]).max() + (HR[t] - end[s]).max()) - p['intron_open']
    top = max(got.values())
    return sorted(k for k, v in got.items() if v == top)


# ---- what ciri_long_amd.seed makes of it ---------------------------------------------------------------------------------------------
# These restate seed.py's own steps (the anchors of a link, the dict of a junction, the circle, the cut of the pieces) and are no
# independent evidence: an equality with them shows that the device rows were carried through unchanged, and would share a mistake such
# as a wrong minus-strand read_pos.  What guards those steps are the planted-truth assertions of tests/test_junction_host.py and
# tests/test_gpu_junction.py on the circle, read_pos, the strand, the signal and the exon boundaries.

def path_tasks(names, path, L, k):
    """per back-splice link of a link_reads path its (contig index, task)"""
    out = []
    for t, name in enumerate(path['links']):
        if name == 'backsplice':
            j, i = path['chains'][t], path['chains'][t + 1]
            y1 = L - j['query_start'] if path['minus'] else j['query_end']
            y0 = L - i['query_end'] if path['minus'] else i['query_start']
            out.append((names.index(path['contig']), (int(path['minus']), j['ref_end'] - k, y1 - k, i['ref_start'] + k, y0 + k, 0)))
    return out


def text_of(codes):
    return ''.join('ACGTN'[c] for c in codes)


def junction_dict(genome, read, c, task, **p):
    """one entry of a refined path's `junctions`"""
    contig = genome.codes[c]
    row = refine(contig, read, task, **p)
    if row[0]:
        return {'status': row[0], 'score': None, 'strand': None, 'circle': None, 'read_pos': None, 'donor': None, 'acceptor': None}
    after, before = contig[row[6]:row[6] + 2], contig[max(row[7] - 2, 0):row[7]]
    donor, acceptor = (sc.revcomp(before), sc.revcomp(after)) if row[2] else (after, before)
    y = task[2] + row[3]
    return {'status': 0, 'score': row[1], 'strand': '+-'[row[2]], 'circle': (genome.names[c], row[7], row[6]), 'read_pos': len(read) - y if task[0] else y,
            'donor': text_of(donor), 'acceptor': text_of(acceptor)}


def refine_paths(genome, read, paths, k, **p):
    """what seed.refine_junctions gives for the paths of one read"""
    out = []
    for path in paths:
        path = dict(path)
        path['junctions'] = [junction_dict(genome, read, c, task, **p) for c, task in path_tasks(genome.names, path, len(read), k)]
        out.append(path)
    return out


def circle_of(path):
    """what seed.call_circles makes of a refined best path, or None"""
    done = [j for j in path['junctions'] if j['status'] == 0]
    if not done:
        return None
    j = max(done, key=lambda v: v['score'])
    contig, start, end = j['circle']
    return {'circ_id': '%s:%d-%d' % (contig, start + 1, end), 'contig': contig, 'start': start, 'end': end, 'strand': j['strand'],
            'signal': '%s-%s' % (j['donor'], j['acceptor']), 'score': j['score'], 'read_pos': j['read_pos'], 'path': path}


def refined_pieces(path):
    """the pieces of a refined path as map_spliced(refine=True) cuts them"""
    pieces = [dict(p) for p in path['pieces']]
    for t, j in enumerate(path['junctions']):
        if j['status'] == 0:
            left, right = pieces[t], pieces[t + 1]
            left['ref_end'], right['ref_start'] = j['circle'][2], j['circle'][1]
            left['query_start' if path['minus'] else 'query_end'] = right['query_end' if path['minus'] else 'query_start'] = j['read_pos']
    return pieces
