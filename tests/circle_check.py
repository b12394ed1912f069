"""The plain statement of K7c (csrc/seed_circle.hip): the circles of a read batch -- the best path of every read, its K7j tasks, the winner
among the refined junctions, the flank codes, the row of 16 words per read and the table of the distinct circles with their read counts.
Written from the definition of include/ciri_long_hip.h on top of tests/link_check.py and tests/junction_check.py; the yardstick of
tests/test_circle_host.py and tests/test_gpu_circles.py (not a test module).

The statement works on the raw chains of a read's two segments (link_check.segment_chains) and on link_check.link's F, pred, kind and
paths, not on the path dicts of link_check.paths_of: tests/test_circle_host.py holds it to those, through junction_check.circle_of."""
import junction_check as jc
import link_check as lc
import seed_check as sc

ROW, TABLE = 16, 10
FOUND, NO_PATH, NO_BACKSPLICE, NO_JUNCTION = 0, 1, 2, 3


def split(params):
    """the keywords of one call -> (chain keywords, link keywords, junction keywords); max_skew is the chain's and the link's"""
    params = dict(params)
    chain = {name: params.pop(name) for name in lc.CHAIN_KEYS if name in params}
    junction = {name: params.pop(name) for name in jc.DEFAULTS if name in params}
    link = params
    link.setdefault('max_skew', chain.get('max_skew', 500))
    assert not set(link) - set(lc.DEFAULTS), link
    return chain, link, junction


def best_path(segments, k, min_path_score=0, **link_p):
    """segments: [plus chains, minus chains] of one read -> (minus, score, walk, kind) of the best path, or None: the candidates are the
    paths of both segments with a score of at least min_path_score, the best is the least under (-score, minus, x_first of the path's
    first chain, path index)"""
    best = None
    for minus, mine in enumerate(segments):
        _, _, kind, paths = lc.link(mine, k, **link_p)
        for index, (score, walk) in enumerate(paths):
            if score >= min_path_score:
                key = (-score, minus, mine[walk[0]]['x_first'], index)
                if best is None or key < best[0]:
                    best = (key, (minus, score, walk, kind))
    return best[1] if best else None


def tasks(r, minus, mine, walk, kind, k):
    """the K7j tasks of a path, in ascending pos: (read, minus, contig, xd, yd, xa, ya, 0) for every chain i with kind 3 and j its predecessor"""
    out = []
    for pos in range(1, len(walk)):
        j, i = mine[walk[pos - 1]], mine[walk[pos]]
        if kind[walk[pos]] == 3:
            out.append((r, minus, i['contig'], j['x_end'] - k, j['y_end'] - k, i['x_first'] + k, i['y_first'] + k, 0))
    return out


def dinucleotide(contig, p):
    """5 c0 + c1 of contig[p : p + 2), -1 where fewer than two of its letters lie inside the contig"""
    if p < 0 or p + 2 > len(contig):
        return -1
    return 5 * contig[p] + contig[p + 1]


def revcomp_code(code):
    if code < 0:
        return -1
    c0, c1 = divmod(code, 5)
    return 5 * (3 - c1 if c1 < 4 else 4) + (3 - c0 if c0 < 4 else 4)


def flanks(contig, start, end, strand):
    """-> (donor code, acceptor code) of the circle [start, end) as the transcript on `strand` (0 +, 1 -) reads them"""
    after, before = dinucleotide(contig, end), dinucleotide(contig, start - 2)
    return (revcomp_code(before), revcomp_code(after)) if strand else (after, before)


def row(genome, read, r, segments, k, min_path_score=0, link_p=None, junction_p=None):
    """the 16 words of read r"""
    best = best_path(segments, k, min_path_score, **(link_p or {}))
    if best is None:
        return [NO_PATH] + [0] * 15
    minus, score, walk, kind = best
    mine = tasks(r, minus, segments[minus], walk, kind, k)
    tail = [minus, score, len(walk), len(mine)]
    if not mine:
        return [NO_BACKSPLICE] + [0] * 8 + tail + [0, 0, 0]
    rows = [jc.refine(genome.codes[t[2]], read, (t[1],) + tuple(t[3:]), **(junction_p or {})) for t in mine]
    done = [o for o, v in enumerate(rows) if v[0] == 0]
    if not done:
        return [NO_JUNCTION] + [0] * 8 + tail + [0, 0, 0]
    w = min(done, key=lambda o: (-rows[o][1], o))          # the greatest J, the first among equals
    t, v = mine[w], rows[w]
    start, end, strand = v[7], v[6], v[2]
    donor, acceptor = flanks(genome.codes[t[2]], start, end, strand)
    y = t[4] + v[3]
    return [FOUND, t[2], start, end, strand, donor, acceptor, v[1], len(read) - y if minus else y] + tail + [len(done), w, 0]


def table(rows):
    """-> (table, circle_of_read): the status-0 rows grouped by (contig, start, end, strand) exactly, ascending; per group contig, start,
    end, strand, donor, acceptor, reads, the greatest J, the lowest read index, 0"""
    groups = {}
    for r, v in enumerate(rows):
        if v[0] == FOUND:
            groups.setdefault(tuple(v[1:5]), []).append(r)
    order = sorted(groups)
    out = [list(key) + rows[groups[key][0]][5:7] + [len(groups[key]), max(rows[r][7] for r in groups[key]), min(groups[key]), 0] for key in order]
    where = {key: g for g, key in enumerate(order)}
    return out, [where[tuple(v[1:5])] if v[0] == FOUND else -1 for v in rows]


def circles(genome, idx, reads, k, w, max_occ, min_path_score=0, **params):
    """what SeedIndex.circles gives for reads (code lists): (circle rows, circle_of_read, table)"""
    chain_p, link_p, junction_p = split(params)
    rows = [row(genome, read, r, lc.segment_chains(genome, idx, read, k, w, max_occ, **chain_p), k, min_path_score, link_p, junction_p)
            for r, read in enumerate(reads)]
    tab, where = table(rows)
    return rows, where, tab


def signal(genome, v):
    """'GT-AG' or the like of a status-0 circle row (or, shifted by one word, a table row): the codes as letters; where a code is -1 the
    letters that remain inside the contig, as seed.refine_junctions reads them"""
    contig, start, end, strand = genome.codes[v[1]], v[2], v[3], v[4]
    after, before = contig[end:end + 2], contig[max(start - 2, 0):start]
    donor, acceptor = (sc.revcomp(before), sc.revcomp(after)) if strand else (after, before)
    for code, letters in ((v[5], donor), (v[6], acceptor)):
        assert (code == -1 and len(letters) < 2) or code == 5 * letters[0] + letters[1], (v, letters)
    return '%s-%s' % (jc.text_of(donor), jc.text_of(acceptor))


def circle_dict(genome, v):
    """a circle row as seed.circle_dicts gives it: seed.call_circles' dict without its path, None without a circle"""
    if v[0] != FOUND:
        return None
    name = genome.names[v[1]]
    return {'circ_id': '%s:%d-%d' % (name, v[2] + 1, v[3]), 'contig': name, 'start': v[2], 'end': v[3], 'strand': '+-'[v[4]], 'signal': signal(genome, v),
            'score': v[7], 'read_pos': v[8]}


def table_dicts(genome, tab):
    """the table as seed.call_circles_batch lists it"""
    return [{'circ_id': '%s:%d-%d' % (genome.names[t[0]], t[1] + 1, t[2]), 'contig': genome.names[t[0]], 'start': t[1], 'end': t[2], 'strand': '+-'[t[3]],
             'signal': signal(genome, [0] + list(t)), 'reads': t[6], 'score': t[7], 'first_read': t[8]} for t in tab]
