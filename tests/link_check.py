"""The plain statement of K7's link step (csrc/seed_link.hip): the chains of one (read, strand) segment linked into paths whose links are
colinear, introns or back-splices, and what ciri_long_amd.seed makes of them (link_reads, link_chains, the pieces map_spliced aligns).
Written from the definitions of include/ciri_long_hip.h with no cleverness, on top of tests/seed_check.py; the yardstick of
tests/test_link_host.py and tests/test_gpu_link.py.

A chain is a dict as seed_check.read_chains gives it: contig (its index), score, x_first, y_first, x_end, y_end (and minus, anchors)."""
import seed_check as sc

DEFAULTS = dict(max_query_gap=500, max_overlap=32, max_skew=500, max_intron=200000, max_circle=200000, intron_cost=16, backsplice_cost=32)
KINDS = {1: 'colinear', 2: 'intron', 3: 'backsplice'}
CHAIN_KEYS = ('lookback', 'max_gap', 'max_skew', 'min_score', 'min_anchors', 'max_chains', 'max_attempts')


def parameters(p):
    unknown = set(p) - set(DEFAULTS)
    assert not unknown, unknown
    out = dict(DEFAULTS)
    out.update(p)
    return out


def key(chains, c):
    return (chains[c]['y_first'], chains[c]['y_end'], chains[c]['x_first'], c)


def ranks(chains):
    order = sorted(range(len(chains)), key=lambda c: key(chains, c))
    rank = [0] * len(chains)
    for r, c in enumerate(order):
        rank[c] = r
    return rank, order


def classify(d, span, p):
    """the kind of a link of skew d = (x0_i - x1_j) - q that goes span = x1_j - x0_i back on the contig: 1, 2, 3, or 0 for none"""
    kinds = []
    if abs(d) <= p['max_skew']:
        kinds.append(1)
    if p['max_skew'] < d <= p['max_intron']:
        kinds.append(2)
    if d < -p['max_skew'] and 0 < span <= p['max_circle']:
        kinds.append(3)
    assert len(kinds) <= 1
    return kinds[0] if kinds else 0


def link_term(cj, ci, k, p):
    """what the link j -> i adds to F_j, (-(cost + read overlap), kind), or None where it is not admissible; rank j < rank i is the caller's"""
    if cj['contig'] != ci['contig'] or not (ci['y_first'] > cj['y_first'] and ci['y_end'] > cj['y_end']):
        return None
    q = ci['y_first'] - cj['y_end']
    if q > p['max_query_gap'] or -q > p['max_overlap']:
        return None
    d = (ci['x_first'] - cj['x_end']) - q
    kind = classify(d, cj['x_end'] - ci['x_first'], p)
    if kind == 0:
        return None
    cost = {1: sc.beta(abs(d), k), 2: p['intron_cost'], 3: p['backsplice_cost']}[kind]
    return -(cost + max(0, -q)), kind


def link(chains, k, **p):
    """-> (F, pred, kind, paths): per chain its F, predecessor (-1) and the kind of the link from it (0); paths [(score, [chains from
    the path's first to its last])] in the order of extraction"""
    p = parameters(p)
    n = len(chains)
    rank, order = ranks(chains)
    F, pred, kind = [None] * n, [-1] * n, [0] * n
    for i in order:
        best = None                                     # (value, rank of j, j, kind)
        for j in order[:rank[i]]:
            t = link_term(chains[j], chains[i], k, p)
            if t is not None and F[j] + t[0] > 0:
                cand = (F[j] + t[0], rank[j], j, t[1])
                if best is None or cand[:2] > best[:2]:
                    best = cand
        F[i] = chains[i]['score'] + (best[0] if best else 0)
        if best:
            pred[i], kind[i] = best[2], best[3]
    used, paths = [False] * n, []
    while not all(used):
        e = min((c for c in range(n) if not used[c]), key=lambda c: (-F[c], rank[c]))
        walk, i = [], e
        while i >= 0 and not used[i]:
            used[i] = True
            walk.append(i)
            i = pred[i]
        paths.append((F[e] - (F[i] if i >= 0 else 0), walk[::-1]))
    return F, pred, kind, paths


def rows(chains, k, **p):
    """the link rows of one segment as the kernel writes them: per chain [rank, F, pred, kind, path, pos, the path's score where pos == 0, 0]"""
    F, pred, kind, paths = link(chains, k, **p)
    rank, _ = ranks(chains)
    out = [None] * len(chains)
    for pi, (score, walk) in enumerate(paths):
        for pos, c in enumerate(walk):
            out[c] = [rank[c], F[c], pred[c], kind[c], pi, pos, score if pos == 0 else 0, 0]
    return out, len(paths)


def segment_chains(genome, idx, read, k, w, max_occ, lookback=64, max_gap=5000, max_skew=500, min_score=40, min_anchors=3, max_chains=32, max_attempts=None):
    """the chains of one read per strand IN THE ORDER THE CHAIN KERNEL EMITS THEM (seed_check.read_chains sorts them): [plus, minus]"""
    anchors, _ = sc.seeds(idx, read, k, w, max_occ)
    out = []
    for minus in (0, 1):
        seg = [(x, y) for m, x, y in anchors if m == minus]
        f, p = sc.chains(seg, genome.contig_of, k, lookback, max_gap, max_skew)
        got, _ = sc.extract(seg, f, p, k, min_score, min_anchors, max_chains, max_attempts)
        mine = []
        for score, count, first, last in got:
            c = genome.contig_of(seg[last][0])
            mine.append({'minus': minus, 'contig': c, 'score': score, 'anchors': count, 'x_first': seg[first][0] - genome.start[c], 'y_first': seg[first][1],
                         'x_end': seg[last][0] - genome.start[c] + k, 'y_end': seg[last][1] + k})
        out.append(mine)
    return out


def map_style(names, c, L, k):
    """a chain as seed.map_reads gives it"""
    name = names[c['contig']]
    if c['minus']:
        qs, qe, anchor = L - c['y_end'], L - c['y_first'], (name, c['x_first'] + k, L - k - c['y_first'])
    else:
        qs, qe, anchor = c['y_first'], c['y_end'], (name, c['x_first'], c['y_first'])
    return {'contig': name, 'minus': bool(c['minus']), 'score': c['score'], 'anchors': c['anchors'], 'ref_start': c['x_first'], 'ref_end': c['x_end'],
            'query_start': qs, 'query_end': qe, 'anchor': anchor}


def path_dict(chains, kinds, score):
    """chains: map_reads-style, in the strand's read order; kinds: the kind of the link into each chain but the first"""
    minus = chains[0]['minus']
    links = [KINDS[v] for v in kinds]
    runs, run = [], [chains[0]]
    for c, name in zip(chains[1:], links):
        if name == 'backsplice':
            runs.append(run)
            run = []
        run.append(c)
    runs.append(run)
    pieces = [{'ref_start': r[0]['ref_start'], 'ref_end': r[-1]['ref_end'], 'query_start': (r[-1] if minus else r[0])['query_start'],
               'query_end': (r[0] if minus else r[-1])['query_end']} for r in runs]
    out = {'contig': chains[0]['contig'], 'minus': minus, 'score': score, 'chains': chains, 'links': links, 'pieces': pieces}
    back = [t for t, name in enumerate(links) if name == 'backsplice']
    if back:
        out['circle'] = (chains[0]['contig'], min(chains[t + 1]['ref_start'] for t in back), max(chains[t]['ref_end'] for t in back))
        first = chains[back[0] + 1]
        out['rotation'] = first['query_end'] if minus else first['query_start']
    return out


def paths_of(segments, names, L, k, min_path_score=0, **p):
    """segments: [plus chains, minus chains] of one read -> its paths as seed.link_reads gives them"""
    out = []
    for mine in segments:
        _, _, kind, paths = link(mine, k, **p)
        for score, walk in paths:
            if score >= min_path_score:
                out.append(path_dict([map_style(names, mine[c], L, k) for c in walk], [kind[c] for c in walk[1:]], score))
    return sorted(out, key=lambda v: (-v['score'], v['minus'], v['chains'][0]['ref_start']))


def link_read(genome, idx, read, k, w, max_occ, min_path_score=0, **params):
    """what seed.link_reads gives for one read (codes)"""
    chain_p = {name: params.pop(name) for name in CHAIN_KEYS if name in params}
    params.setdefault('max_skew', chain_p.get('max_skew', 500))
    return paths_of(segment_chains(genome, idx, read, k, w, max_occ, **chain_p), genome.names, len(read), k, min_path_score, **params)


def raw_of(names, c, L):
    """a map_reads-style chain back as the chain of its strand"""
    y0, y1 = (L - c['query_end'], L - c['query_start']) if c['minus'] else (c['query_start'], c['query_end'])
    return {'minus': int(c['minus']), 'contig': names.index(c['contig']), 'score': c['score'], 'anchors': c.get('anchors', 0), 'x_first': c['ref_start'],
            'y_first': y0, 'x_end': c['ref_end'], 'y_end': y1}


def link_chains(names, chain_lists, read_lengths, k, min_path_score=0, **p):
    """what seed.link_chains gives: per read the paths of its caller-given map_reads-style chains, each strand in the order given"""
    out = []
    for mine, L in zip(chain_lists, read_lengths):
        raw = [raw_of(names, c, L) for c in mine]
        out.append(paths_of([[c for c in raw if c['minus'] == m] for m in (0, 1)], names, L, k, min_path_score, **p))
    return out


def spliced_pieces(path, read):
    """the windows and queries map_spliced aligns for one path: per piece ((contig, ref_start, ref_end), the strand's read letters)"""
    out = []
    for piece in path['pieces']:
        q = list(read[piece['query_start']:piece['query_end']])
        out.append(((path['contig'], piece['ref_start'], piece['ref_end']), sc.revcomp(q) if path['minus'] else q))
    return out
