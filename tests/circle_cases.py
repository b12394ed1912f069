"""The planted inputs of tests/test_circle_host.py (asserted with the checker tests/circle_check.py alone) and tests/test_gpu_circles.py
(the same reads asked of the GPU): the world and the reads of tests/junction_cases.py, and beside them small contigs of one exon each
and reads planted for the cases K7c has to tell apart -- a read without a path, a linear read, a best path without a back-splice above
a lower one with one, junctions too wide to refine, strands that tie, two turns of a circle, circles that touch a contig's end, flanks
with N and lower-case letters, one circle read on both strands, one pair of coordinates on two contigs that read it on either
transcript strand, and a run of junction widths across the K7j class bound at 64."""
import functools
import random

import circle_check as cc
import junction_cases as jcases
import seed_check as sc

K, W, MAX_OCC = jcases.K, jcases.W, jcases.MAX_OCC
# junction_cases' link parameters; max_query_gap above max_span + what the anchors add, so that a link can be too wide to refine
LINK = dict(jcases.LINK, max_query_gap=600)
# a scoring away from every default: unit match, dearer mismatches and gaps, free intron_open, a cheap GC donor, no slack; under its
# max_span of 40 most planted junk is too wide to refine
SCORING = dict(match=1, mismatch=3, gap_open=4, gap_extend=2, intron_open=0, noncanonical=2, donor_costs={'GC': 1}, slack=0, max_span=40)
dna, rc = jcases.dna, jcases.rc


def exon(rng, n):
    return rng.choice('AT') + dna(rng, n - 2) + rng.choice('AT')


@functools.lru_cache(maxsize=None)
def world():
    """-> (contigs [(name, text)], spots {name: (start, end)} of the one exon of each new contig): junction_cases' four contigs, then
    e0 (the exon ends the contig), e1 (it begins it), n0 ('ag' in lower case in front, 'GN' behind), p0 and m0 (one layout, other
    letters: AG..GT around the one, AC..CT around the other)"""
    contigs = list(jcases.world()[0])
    rng = random.Random(61)
    spots = {}

    def add(name, head, body, tail):
        spots[name] = (len(head), len(head) + len(body))
        contigs.append((name, head + body + tail))
    add('e0', dna(rng, 200) + 'AG', exon(rng, 260), '')
    add('e1', '', exon(rng, 260), 'GT' + dna(rng, 200))
    add('n0', dna(rng, 150).upper() + 'ag', exon(rng, 250), 'GN' + dna(rng, 150))
    add('p0', dna(rng, 150) + 'AG', exon(rng, 240), 'GT' + dna(rng, 150))
    add('m0', dna(rng, 150) + 'AC', exon(rng, 240), 'CT' + dna(rng, 150))
    assert spots['p0'] == spots['m0'] and max(len(t) for _, t in contigs) <= 4096
    return contigs, spots


def turn(name, cut, junk=''):
    """one copy of the exon of `name`, begun `cut` letters in, `junk` between its end and its start"""
    contigs, spots = world()
    a, b = spots[name]
    body = dict(contigs)[name][a:b]
    return body[cut:] + junk + body[:cut]


@functools.lru_cache(maxsize=None)
def reads():
    """-> [(label, text)]: junction_cases' 24 reads first, then the planted ones"""
    contigs, spots = world()
    text_of = dict(contigs)
    rng = random.Random(62)
    base = jcases.reads()
    out = [('junction_cases %d' % r, v['text']) for r, v in enumerate(base)]
    out.append(('empty', ''))
    out.append(('random', dna(rng, 300)))
    out.append(('linear', text_of['j0'][150:700]))
    out.append(('linear minus', rc(text_of['j2'][300:800])))
    out.append(('linear above circle', text_of['j1'][100:760] + turn('e0', 120)))
    out.append(('too wide', turn('p0', 100, dna(rng, 530))))
    clean = [v['text'] for v in base if not v['errors']]
    out.append(('palindrome a', clean[0] + rc(clean[0])))
    out.append(('palindrome b', clean[9] + rc(clean[9])))
    a, b = spots['p0']
    body = text_of['p0'][a:b]
    out.append(('two turns equal', body[130:] + body + body[:90]))
    hit = body[:6] + {'A': 'C', 'C': 'G', 'G': 'T', 'T': 'A'}[body[6]] + body[7:90]     # a substitution 6 letters behind the second junction
    out.append(('two turns second wins', body[130:] + body + hit))
    out.append(('contig end', turn('e0', 140)))
    out.append(('contig end minus', rc(turn('e0', 90))))
    out.append(('contig start', turn('e1', 110)))
    out.append(('n and lower case', turn('n0', 100)))
    out.append(('n and lower case minus', rc(turn('n0', 160))))
    out.append(('plus transcript', turn('p0', 115)))
    out.append(('minus transcript', turn('m0', 115)))
    out.append(('minus transcript minus', rc(turn('m0', 70))))
    for width in range(18, 49):                         # m = width + 2 k + what the sketch leaves between the anchors and the exon's ends
        out.append(('width %d' % width, turn('m0', 100 + width, dna(rng, width))))
    return out


def texts():
    return [t for _, t in reads()]


def label(name):
    return [r for r, (lab, _) in enumerate(reads()) if lab == name][0]


def link_of(max_chains=None):
    """LINK, with another max_chains where one is given"""
    return dict(LINK) if max_chains is None else dict(LINK, max_chains=max_chains)


@functools.lru_cache(maxsize=None)
def indexed():
    """-> (sc.Genome, its index)"""
    genome = sc.Genome(world()[0])
    return genome, sc.index(genome.codes, K, W)


@functools.lru_cache(maxsize=None)
def checked():
    """-> (sc.Genome, its index, per read the checker's link_reads paths at LINK): computed once"""
    genome, idx = indexed()
    return genome, idx, [jcases.lc.link_read(genome, idx, sc.encode(t), K, W, MAX_OCC, **dict(LINK)) for t in texts()]


@functools.lru_cache(maxsize=None)
def refined(scoring=False):
    """-> per read the checker's refine_junctions paths, at the default scoring or at SCORING"""
    genome, _, paths = checked()
    return [jcases.jc.refine_paths(genome, sc.encode(t), mine, K, **(SCORING if scoring else {})) for t, mine in zip(texts(), paths)]


@functools.lru_cache(maxsize=None)
def segments(max_chains=None):
    """-> per read the raw chains of its two segments at LINK's chain parameters (max_chains: another than LINK's)"""
    genome, idx = indexed()
    chain_p, _, _ = cc.split(link_of(max_chains))
    return [jcases.lc.segment_chains(genome, idx, sc.encode(t), K, W, MAX_OCC, **chain_p) for t in texts()]


@functools.lru_cache(maxsize=None)
def want(scoring=False, min_path_score=0, max_chains=None):
    """-> (circle rows, circle_of_read, table) of the planted reads by the checker (max_chains: another than LINK's)"""
    genome, _ = indexed()
    _, link_p, junction_p = cc.split(dict(link_of(max_chains), **(SCORING if scoring else {})))
    rows = [cc.row(genome, sc.encode(t), r, segs, K, min_path_score, link_p, junction_p)
            for r, (t, segs) in enumerate(zip(texts(), segments(max_chains)))]
    tab, where = cc.table(rows)
    return rows, where, tab
