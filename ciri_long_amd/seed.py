"""Reads to loci on the device (K7): a minimizer index of the resident genome, seed look-up and colinear chaining, offered beside the
external mapper -- nothing in find_bsj.py or mapper_pool.py is routed through it.  A chain names a contig, a strand and the two spans
it covers, and its first anchor in the form ``ssw_wrap.extend_anchors_genome`` takes, so that
``reads -> map_reads -> extend_anchors_genome / align_windows_spliced`` stays on the device from letters to CIGARs.

The definitions (minimizers with all ties selected, anchors, chain score, extraction) are the project's own and are not those of
minimap2: include/ciri_long_hip.h states them, tests/seed_check.py restates them in plain Python.

One chain comes out per exon.  ``link_reads`` links the chains of a read into paths across introns and back-splice junctions, still on
the device (csrc/seed_link.hip; tests/link_check.py is its plain statement), and ``map_spliced`` carries the best path through
``ssw_wrap.align_windows_spliced``: ``reads -> chains -> paths -> exons and circle`` with no external mapper and no host loop over
rotations of the read.  ``refine_junctions`` names every back-splice junction of a path to the base (csrc/seed_junction.hip, K7j;
tests/junction_check.py is its plain statement), ``call_circles`` makes ``contig:start-end`` with strand and splice signal of it, and
``map_spliced(refine=True)`` cuts the pieces there."""
import numpy as np

from . import hip


def index(genome, k=15, w=5, max_occ=64):
    """the minimizer index of a ``hip.Genome``: every contig sketched as a sequence of its own, entries sorted by (key, position);
    a key with more than max_occ entries seeds nothing"""
    return hip.SeedIndex(genome, k=k, w=w, max_occ=max_occ)


def _map_style(index, c, L):
    """a chain of SeedIndex.chains (or a chain row as a dict) of a read of L letters as map_reads gives it"""
    name, k = index.contigs[c['contig']], index.k
    if c['minus']:
        qs, qe = L - c['y_end'], L - c['y_first']
        anchor = (name, c['x_first'] + k, L - k - c['y_first'])
    else:
        qs, qe = c['y_first'], c['y_end']
        anchor = (name, c['x_first'], c['y_first'])
    return {'contig': name, 'minus': bool(c['minus']), 'score': c['score'], 'anchors': c['anchors'], 'ref_start': c['x_first'],
            'ref_end': c['x_end'], 'query_start': qs, 'query_end': qe, 'anchor': anchor}


def map_reads(index, reads, **chain_parameters):
    """reads: a list of str / int8 code arrays.  Per read the list of its chains, best first (``SeedIndex.chains`` and its parameters:
    lookback, max_gap, max_skew, min_score, min_anchors, max_chains, max_attempts), each a dict:

    contig, minus          the contig's name; True where the read maps to the minus strand
    score, anchors         the chain's score and its number of anchors
    ref_start, ref_end     the span of the contig from the first anchor's k-mer to the last one's
    query_start, query_end the span of the read AS GIVEN (on the minus strand converted back from the reverse-complemented read)
    anchor                 the chain's first anchor (lowest on the contig) as ``extend_anchors_genome`` takes it, (contig, pos,
                           query_pos): a plus-strand hit of read k-mer q on genome k-mer g is (contig, g, q); a minus-strand hit is
                           (contig, g + k, q), read position q facing the upper edge of the genome k-mer"""
    data, off = hip._packed(reads)
    chains, _ = index.chains((data, off), **chain_parameters)
    return [[_map_style(index, c, int(off[r + 1] - off[r])) for c in mine] for r, mine in enumerate(chains)]


LINK_KINDS = {1: 'colinear', 2: 'intron', 3: 'backsplice'}
_ROW = ('read', 'minus', 'contig', 'score', 'anchors', 'x_first', 'y_first', 'x_end', 'y_end')
_LINK_KEYS = ('max_query_gap', 'max_overlap', 'max_skew', 'max_intron', 'max_circle', 'intron_cost', 'backsplice_cost')
_ALIGN_KEYS = ('match', 'mismatch', 'gap_open', 'gap_extend', 'intron_open', 'noncanonical', 'donor_costs', 'acceptor_costs', 'traceback')


def _path(chains, kinds, score):
    """one path: its map_reads-style chains in the strand's read order and the kind of the link into each chain but the first"""
    minus = chains[0]['minus']
    links = [LINK_KINDS[int(v)] for v in kinds]
    runs = [[chains[0]]]
    for c, name in zip(chains[1:], links):
        if name == 'backsplice':
            runs.append([])
        runs[-1].append(c)
    pieces = [{'ref_start': run[0]['ref_start'], 'ref_end': run[-1]['ref_end'], 'query_start': (run[-1] if minus else run[0])['query_start'],
               'query_end': (run[0] if minus else run[-1])['query_end']} for run in runs]
    path = {'contig': chains[0]['contig'], 'minus': minus, 'score': score, 'chains': chains, 'links': links, 'pieces': pieces}
    back = [t for t, name in enumerate(links) if name == 'backsplice']
    if back:
        path['circle'] = (path['contig'], min(chains[t + 1]['ref_start'] for t in back), max(chains[t]['ref_end'] for t in back))
        target = chains[back[0] + 1]
        path['rotation'] = target['query_end'] if minus else target['query_start']
    return path


def _paths(index, counts, rows, link_rows, lengths, min_path_score):
    """the raw arrays of SeedIndex.links / link_rows (segment 2 r + minus) -> per read its paths, best first"""
    out = []
    for r, L in enumerate(lengths):
        mine = []
        for s in (2 * r, 2 * r + 1):
            n = int(counts[s])
            lr = link_rows[s, :n]
            for p in range(int(lr[:, 4].max()) + 1 if n else 0):
                walk = sorted(np.flatnonzero(lr[:, 4] == p).tolist(), key=lambda c: int(lr[c, 5]))
                score = int(lr[walk[0], 6])
                if score >= min_path_score:
                    chains = [_map_style(index, dict(zip(_ROW, (int(v) for v in rows[s, c, :9]))), L) for c in walk]
                    mine.append(_path(chains, [lr[c, 3] for c in walk[1:]], score))
        out.append(sorted(mine, key=lambda v: (-v['score'], v['minus'], v['chains'][0]['ref_start'])))
    return out


def link_reads(index, reads, min_path_score=0, **parameters):
    """map_reads, and the chains of each (read, strand) linked on the device into paths whose links are colinear, introns or
    back-splices (``SeedIndex.links`` and its parameters: those of map_reads with max_chains=32, and max_query_gap, max_overlap,
    max_intron, max_circle, intron_cost, backsplice_cost; max_skew is the chain's and the link's).  Per read the list of its paths over
    both strands with a score of at least min_path_score, ordered by (-score, minus, ref_start of the first chain), each a dict:

    contig, minus, score   of the path; the score is that of its last chain's F less what the walk stopped on
    chains                 map_reads-style dicts in the strand's read order (on the minus strand: descending in the read as given)
    links                  'colinear' | 'intron' | 'backsplice', one fewer than chains
    pieces                 the maximal runs of chains between back-splice links, each with ref_start (of its first chain), ref_end
                           (of its last), query_start, query_end (in the read as given)
    circle, rotation       only with at least one back-splice: (contig, the lowest ref_start of a back-splice's target, the highest
                           ref_end of a back-splice's source), and the position in the read as given at which the first back-splice's
                           target begins: what find_bsj's rotate-and-map-again loop converges towards, with no mapper call."""
    data, off = hip._packed(reads)
    got = index.links((data, off), **parameters)
    return _paths(index, got['seg'][:, 0], got['rows'], got['link_rows'], np.diff(off).tolist(), min_path_score)


def link_chains(index, chain_lists, read_lengths, min_path_score=0, **link_parameters):
    """link_reads for chains the caller gives (another mapper's hits), through ``SeedIndex.link_rows``: chain_lists[r] holds the
    map_reads-style dicts of read r (contig, minus, score, ref_start, ref_end, query_start, query_end; anchors if known), each strand's in
    the order given, which is the order ties fall back on; read_lengths[r] its length.  At most 64 chains per (read, strand)."""
    n = len(chain_lists)
    if len(read_lengths) != n:
        raise ValueError('link_chains: %d chain lists vs %d read lengths' % (n, len(read_lengths)))
    segs = [[c for c in mine if bool(c['minus']) == bool(s & 1)] for mine in chain_lists for s in (0, 1)]
    most = max([len(s) for s in segs] + [1])
    if most > 64:
        raise ValueError('link_chains: %d chains in one (read, strand), at most 64 are linked' % most)
    rows = np.zeros((2 * n, most, 10), dtype=np.int64)
    for s, mine in enumerate(segs):
        L = int(read_lengths[s >> 1])
        for c, v in enumerate(mine):
            y0, y1 = (L - v['query_end'], L - v['query_start']) if s & 1 else (v['query_start'], v['query_end'])
            rows[s, c, :9] = (s >> 1, s & 1, index.contigs.index(v['contig']), v['score'], v.get('anchors', 0), v['ref_start'], y0, v['ref_end'], y1)
    counts = np.array([len(s) for s in segs], dtype=np.int64)
    got = index.link_rows(counts, rows, **link_parameters)
    return _paths(index, counts, rows, got['link_rows'], [int(v) for v in read_lengths], min_path_score)


_JUNCTION_KEYS = ('match', 'mismatch', 'gap_open', 'gap_extend', 'intron_open', 'noncanonical', 'donor_costs', 'acceptor_costs', 'slack', 'max_span')
_COMPLEMENT = str.maketrans('ACGT', 'TGCA')


def _junction_tasks(index, number, r, L, path):
    """the task rows of SeedIndex.junctions for the back-splice links of one path of read r (L letters): the donor anchor is the start
    of the source chain's last k-mer, the acceptor anchor the end of the target chain's first k-mer, both strands asked for; number:
    contig name -> index"""
    k, minus, out = index.k, path['minus'], []
    for t, name in enumerate(path['links']):
        if name == 'backsplice':
            j, i = path['chains'][t], path['chains'][t + 1]
            y1_j = L - j['query_start'] if minus else j['query_end']
            y0_i = L - i['query_end'] if minus else i['query_start']
            out.append((r, int(minus), number[path['contig']], j['ref_end'] - k, y1_j - k, i['ref_start'] + k, y0_i + k, 0))
    return out


def refine_junctions(index, reads, paths, **scoring):
    """paths: what ``link_reads`` gave for these reads.  Every back-splice link of every path is refined to the base on the device
    (``SeedIndex.junctions`` and its scoring keywords; K7j, the definition: include/ciri_long_hip.h) in one batch.  -> the paths, each
    with ``junctions``: one dict per back-splice link, in the path's order:

    status          0 refined; 1 more than max_span read letters between the anchors; 2 the anchors cross (then the rest is None)
    score, strand   J of the definition; '+' / '-', the transcript's strand, from the splice signals
    circle          (contig, acceptor_start, donor_end): the circle's 0-based start and exclusive end
    read_pos        the split in the read as given: the first read_pos letters lie on one side of the junction
    donor, acceptor the dinucleotides beside the circle as the transcript reads them, 'GT' and 'AG' at a canonical junction"""
    data, off = hip._packed(reads)
    lengths = np.diff(off).tolist()
    out = [[dict(path) for path in mine] for mine in paths]
    tasks, where = [], []
    number = {name: c for c, name in enumerate(index.contigs)}
    for r, mine in enumerate(out):
        for path in mine:
            path['junctions'] = []
            for task in _junction_tasks(index, number, r, lengths[r], path):
                tasks.append(task)
                where.append(path)
    if not tasks:
        return out
    rows = index.junctions((data, off), np.array(tasks, dtype=np.int64), **scoring)
    windows = []
    for task, row in zip(tasks, rows.tolist()):
        if row[0] == 0:
            name = index.contigs[task[2]]
            size = index.genome.length[name]
            windows += [(name, row[6], min(row[6] + 2, size)), (name, max(row[7] - 2, 0), row[7])]
    flanks = iter(index.genome.letters(windows) if windows else [])
    for task, row, path in zip(tasks, rows.tolist(), where):
        if row[0] != 0:
            path['junctions'].append({'status': row[0], 'score': None, 'strand': None, 'circle': None, 'read_pos': None, 'donor': None, 'acceptor': None})
            continue
        after, before = next(flanks), next(flanks)
        if row[2]:
            donor, acceptor = before.translate(_COMPLEMENT)[::-1], after.translate(_COMPLEMENT)[::-1]
        else:
            donor, acceptor = after, before
        y = task[4] + row[3]
        path['junctions'].append({'status': 0, 'score': row[1], 'strand': '-' if row[2] else '+', 'circle': (path['contig'], row[7], row[6]),
                                  'read_pos': lengths[task[0]] - y if task[1] else y, 'donor': donor, 'acceptor': acceptor})
    return out


def call_circles(index, reads, **parameters):
    """reads -> circles with no external mapper: ``link_reads`` (its parameters), then the back-splice junctions of each read's best path
    refined (``refine_junctions`` and its scoring keywords).  Per read None where it has no path or no refined junction, else a dict from
    the best-scoring refined junction of that path (the first among equals): circ_id 'contig:start-end' (1-based, inclusive), contig,
    start (0-based), end (exclusive), strand, signal ('GT-AG' or the like: donor-acceptor as the transcript reads them), score, read_pos and
    path (the refined path)."""
    scoring = {name: parameters.pop(name) for name in _JUNCTION_KEYS if name in parameters}
    data, off = hip._packed(reads)
    best = [paths[:1] for paths in link_reads(index, (data, off), **parameters)]
    out = []
    for mine in refine_junctions(index, (data, off), best, **scoring):
        done = [j for j in mine[0]['junctions'] if j['status'] == 0] if mine else []
        if not done:
            out.append(None)
            continue
        j = max(done, key=lambda v: v['score'])
        contig, start, end = j['circle']
        out.append({'circ_id': '%s:%d-%d' % (contig, start + 1, end), 'contig': contig, 'start': start, 'end': end, 'strand': j['strand'],
                    'signal': '%s-%s' % (j['donor'], j['acceptor']), 'score': j['score'], 'read_pos': j['read_pos'], 'path': mine[0]})
    return out


def _signals(index, rows):
    """rows [m, >= 6] of contig, start, end, strand, donor code, acceptor code (a circle row from word 1, or a table row) -> 'GT-AG' or
    the like per row.  A code is 5 c0 + c1; -1 stands where the dinucleotide leaves the contig, and the letters that remain inside it are
    then read from the resident genome as ``refine_junctions`` reads them"""
    text = [['ACGTN'[c // 5] + 'ACGTN'[c % 5] if c >= 0 else None for c in (int(row[4]), int(row[5]))] for row in rows]
    windows, where = [], []
    for t, row in enumerate(rows):
        if None in text[t]:
            name = index.contigs[int(row[0])]
            windows += [(name, int(row[2]), min(int(row[2]) + 2, index.genome.length[name])), (name, max(int(row[1]) - 2, 0), int(row[1]))]
            where.append(t)
    flanks = iter(index.genome.letters(windows) if windows else [])
    for t in where:
        after, before = next(flanks), next(flanks)
        text[t] = [before.translate(_COMPLEMENT)[::-1], after.translate(_COMPLEMENT)[::-1]] if rows[t][3] else [after, before]
    return ['%s-%s' % (d, a) for d, a in text]


def call_circles_batch(index, reads, **parameters):
    """reads -> the sample's circles in one device pass (``SeedIndex.circles`` and its keywords: those of ``link_reads`` with
    min_path_score, and the scoring keywords of ``refine_junctions``; K7c, the definition: include/ciri_long_hip.h).  The reads are
    uploaded once and neither paths nor tasks come back.  -> the dict of arrays of ``SeedIndex.circles`` (circle [n, 16],
    circle_of_read [n], table [n_circles, 10], kernel_ms), and under 'circles' the table as a list of dicts, ascending in (contig, start,
    end, strand): circ_id 'contig:start-end' (1-based, inclusive), contig, start (0-based), end (exclusive), strand, signal, reads (how
    many reads of the batch name this circle), score (the greatest J among them) and first_read (the lowest of their indices).  A
    read's circle is the one ``call_circles`` gives it; ``circle_dicts`` turns the rows into its dicts."""
    got = index.circles(hip._packed(reads), **parameters)
    table = got['table']
    out = dict(got)
    out['circles'] = [{'circ_id': '%s:%d-%d' % (index.contigs[int(row[0])], int(row[1]) + 1, int(row[2])), 'contig': index.contigs[int(row[0])], 'start': int(row[1]),
                       'end': int(row[2]), 'strand': '-' if row[3] else '+', 'signal': signal, 'reads': int(row[6]), 'score': int(row[7]), 'first_read': int(row[8])}
                      for row, signal in zip(table, _signals(index, table))]
    return out


def circle_dicts(index, result):
    """what ``call_circles_batch`` (or ``SeedIndex.circles``) gave -> per read None, or the dict ``call_circles`` gives without its 'path'"""
    rows = result['circle']
    found = [r for r in range(len(rows)) if rows[r, 0] == 0]
    out = [None] * len(rows)
    for r, signal in zip(found, _signals(index, [rows[r, 1:] for r in found])):
        contig, start, end = index.contigs[int(rows[r, 1])], int(rows[r, 2]), int(rows[r, 3])
        out[r] = {'circ_id': '%s:%d-%d' % (contig, start + 1, end), 'contig': contig, 'start': start, 'end': end, 'strand': '-' if rows[r, 4] else '+',
                  'signal': signal, 'score': int(rows[r, 7]), 'read_pos': int(rows[r, 8])}
    return out


def map_spliced(index, reads, context=None, refine=False, **parameters):
    """reads -> chains -> paths -> exons: link_reads (its parameters), then for the best path of each read every piece aligned between
    its outer anchors -- the query is the strand's read letters from the start of the piece's first chain to the end of its last, the
    window (contig, ref_start, ref_end) of the piece -- all pieces of all reads in one ``ssw_wrap.align_windows_spliced(mode='global',
    strand='both', report_cigar=True)`` (its scoring keywords pass through).  Per read None where it has no path, else its best path
    with, on every piece, exons [(start, end)] (inclusive, forward strand), strand ('+' / '-': the transcript's, from the splice
    signals), score and cigar_string; a piece whose ref_end lies below its ref_start (chains that run backwards inside a colinear
    link's skew) is not aligned and carries None.

    By default the ends of a piece are those of its outer anchors and are not refined: a back-splice junction lies up to w - 1 + the
    letters an error took beyond them.  refine=True refines every back-splice of the best path first (``refine_junctions`` with the
    alignment's scoring keywords, and slack, max_span): the path carries ``junctions``, and a piece that ends at a refined back-splice
    (status 0) ends at its donor_end and at the split in the read, the piece behind it begins at acceptor_start and the split, so that
    the exons of a circle tile it to the base; each piece is then aligned as before."""
    from . import ssw_wrap
    junction = {name: parameters.pop(name) for name in ('slack', 'max_span') if refine and name in parameters}      # without refine: unknown keywords, as before
    align = {name: parameters.pop(name) for name in _ALIGN_KEYS if name in parameters}
    data, off = hip._packed(reads)
    best = [dict(paths[0]) if paths else None for paths in link_reads(index, (data, off), **parameters)]
    if refine:
        junction.update({name: v for name, v in align.items() if name in _JUNCTION_KEYS})
        best = [mine[0] if mine else None for mine in refine_junctions(index, (data, off), [[p] if p else [] for p in best], **junction)]
        for path in best:
            if path is None:
                continue
            path['pieces'] = [dict(p) for p in path['pieces']]
            for t, j in enumerate(path['junctions']):
                if j['status'] == 0:
                    left, right = path['pieces'][t], path['pieces'][t + 1]
                    left['ref_end'], right['ref_start'] = j['circle'][2], j['circle'][1]
                    left['query_start' if path['minus'] else 'query_end'] = right['query_end' if path['minus'] else 'query_start'] = j['read_pos']
    windows, queries, where = [], [], []
    for r, path in enumerate(best):
        if path is None:
            continue
        path['pieces'] = [dict(p, exons=None, strand=None, score=None, cigar_string=None) for p in path['pieces']]
        for piece in path['pieces']:
            if piece['ref_end'] < piece['ref_start']:
                continue
            q = data[off[r] + piece['query_start']:off[r] + piece['query_end']]
            queries.append(np.where(q < 4, 3 - q, q)[::-1].astype(np.int8) if path['minus'] else q)
            windows.append((path['contig'], piece['ref_start'], piece['ref_end']))
            where.append(piece)
    got = ssw_wrap.align_windows_spliced(index.genome, windows, queries, mode='global', strand='both', report_cigar=True, context=context, **align)
    for piece, res in zip(where, got):
        piece.update(exons=res.exons, strand=res.strand, score=res.score, cigar_string=res.cigar_string)
    return best
