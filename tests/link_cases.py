"""The planted inputs that tests/test_link_host.py asserts with the checker alone and tests/test_gpu_link.py then asks the GPU about:
genomes of three contigs with genes of 2-5 exons, reads that are one copy of a circle of consecutive exons, rotated, on either strand,
error-free and with 8 % errors, and linear transcripts; and the checker's view of them (seed_check / link_check), computed once."""
import functools
import random

import link_check as lc
import seed_check as sc

K, W, MAX_OCC = 15, 5, 64


def dna(rng, n):
    return ''.join(rng.choice('ACGT') for _ in range(n))


def rc(text):
    return text[::-1].translate(str.maketrans('ACGTacgt', 'TGCAtgca'))


def mutate(rng, text, rate):
    out = []
    for ch in text:
        u = rng.random()
        if u < rate / 3:
            out.append(rng.choice([c for c in 'ACGT' if c != ch.upper()]))
        elif u < 2 * rate / 3:
            out.append(ch + rng.choice('ACGT'))
        elif u >= rate:
            out.append(ch)
    return ''.join(out)


def chain(contig, score, x0, x1, y0, y1):
    """a planted chain row as the checker takes it"""
    return {'minus': 0, 'contig': contig, 'score': score, 'anchors': 3, 'x_first': x0, 'y_first': y0, 'x_end': x1, 'y_end': y1}


def gene(rng, strand):
    """-> (text, exons [(start, end)] inside it, end exclusive): 2-5 exons of 120-400 letters, one of them at least 220 so that a rotation
    can leave 100 letters on either side; introns of 600-3000 letters, above the chain's max_skew, that read GT..AG on the gene's strand
    (CT..AC on the contig for a gene on '-').  Every exon begins and ends with A or T, so no intron can slide along a shared letter."""
    n = rng.randint(2, 5)
    lens = [rng.randint(120, 400) for _ in range(n)]
    if max(lens) < 220:
        lens[rng.randrange(n)] = rng.randint(220, 400)
    text, exons = '', []
    for e, ln in enumerate(lens):
        if e:
            inner = dna(rng, rng.randint(600, 3000) - 4)
            text += ('GT' + inner + 'AG') if strand == '+' else ('CT' + inner + 'AC')
        exons.append((len(text), len(text) + ln))
        text += rng.choice('AT') + dna(rng, ln - 2) + rng.choice('AT')
    return text, exons


@functools.lru_cache(maxsize=None)
def world(seed=7):
    """-> (contigs [(name, text)], genes [(contig, strand, exons in contig coordinates)]): three contigs, five genes, at most 40 kb"""
    rng = random.Random(seed)
    contigs, genes = [], []
    for c, count in enumerate((2, 2, 1)):
        text = dna(rng, 300)
        for g in range(count):
            strand = '+-'[(c + g) & 1]
            body, exons = gene(rng, strand)
            genes.append(('g%d' % c, strand, [(len(text) + a, len(text) + b) for a, b in exons]))
            text += body + dna(rng, 300)
        contigs.append(('g%d' % c, text))
    assert sum(len(t) for _, t in contigs) <= 40000
    return contigs, genes


@functools.lru_cache(maxsize=None)
def reads(seed=7):
    """-> [dict]: text, what ('circle' | 'linear'), errors, minus (the read's strand), gene, exons (the planted exons the read holds, in
    contig coordinates, ascending), split (the exon the rotation cuts, or None where it falls between two exons or the read is linear), first
    (the exon the read begins in), junction (where, read along the contig's strand, the circle's first exon begins in an error-free read)"""
    contigs, genes = world(seed)
    text_of = dict(contigs)
    rng = random.Random(seed + 1)
    out = []
    for gi, (name, strand, exons) in enumerate(genes):
        ctg = text_of[name]
        for variant in range(5):
            a = rng.randrange(0, len(exons) - 1)
            b = rng.randrange(a + 1, len(exons))
            if variant < 3 and not any(e1 - e0 >= 220 for e0, e1 in exons[a:b + 1]):
                a, b = 0, len(exons) - 1
            mine = exons[a:b + 1]
            circ = ''.join(ctg[e0:e1] for e0, e1 in mine)
            split = None
            if variant < 3:                             # a circle, rotated inside an exon, 100 letters or more from both its ends
                split = rng.choice([t for t, (e0, e1) in enumerate(mine) if e1 - e0 >= 220])
                e0, e1 = mine[split]
                r = sum(y - x for x, y in mine[:split]) + rng.randint(100, e1 - e0 - 100)
            elif variant == 3:                          # a circle, rotated on the boundary in front of its second exon
                r = mine[0][1] - mine[0][0]
            else:
                r = 0                                   # linear: the exons in order
            text = circ[r:] + circ[:r]
            errors = variant == 2
            if errors:
                text = mutate(rng, text, 0.08)
            minus = bool((gi + variant) & 1)
            out.append({'text': rc(text) if minus else text, 'what': 'linear' if variant == 4 else 'circle', 'errors': errors, 'minus': minus, 'gene': gi,
                        'contig': name, 'exons': mine, 'split': split, 'first': 1 if variant == 3 else (split or 0), 'junction': len(circ) - r})
    return out


@functools.lru_cache(maxsize=None)
def checked(seed=7):
    """-> (sc.Genome, its index, per read the checker's paths): the checker's whole view, computed once"""
    contigs, _ = world(seed)
    genome = sc.Genome(contigs)
    idx = sc.index(genome.codes, K, W)
    return genome, idx, [lc.link_read(genome, idx, sc.encode(r['text']), K, W, MAX_OCC) for r in reads(seed)]


def expected_pieces(read):
    """for an error-free read: per piece the planted exons it holds, as (start, end) inclusive, the cut ends of a split exon open (None)"""
    mine = [(a, b - 1) for a, b in read['exons']]
    if read['what'] == 'linear':
        return [mine]
    f = read['first']
    if read['split'] is None:
        return [mine[f:], mine[:f]]
    return [[(None, mine[f][1])] + mine[f + 1:], mine[:f] + [(mine[f][0], None)]]


# ---- planted chain rows: thresholds, ties, path shapes, fuzz ---------------------------------------------------------------------

def pair(q, d, n=60, contigs=(0, 0), scores=(100, 80)):
    """chain j that ends at (x 300000, y 1000) and chain i that begins q letters further on in the read and q + d further on the contig"""
    x0, y0 = 300000 + q + d, 1000 + q
    return [chain(contigs[0], scores[0], 299000, 300000, 0, 1000), chain(contigs[1], scores[1], x0, x0 + n, y0, y0 + n)]


def threshold_cases():
    """[(label, chains, parameters, the kind the link 0 -> 1 must have, 0 for none)] at the defaults but for what the label says"""
    D = lc.DEFAULTS
    skew, intron, circle, gap, over = D['max_skew'], D['max_intron'], D['max_circle'], D['max_query_gap'], D['max_overlap']
    out = [('d = %d' % d, pair(10, d), {}, kind) for d, kind in ((skew, 1), (-skew, 1), (skew + 1, 2), (-skew - 1, 3), (intron, 2), (intron + 1, 0), (0, 1))]
    # the circle's span x1_j - x0_i = -(q + d); with max_skew 100 and q = 200 a span of 0 is still d < -max_skew
    out += [('span %d' % s, pair(200, -200 - s), {'max_skew': 100}, kind) for s, kind in ((0, 0), (1, 3), (circle, 3), (circle + 1, 0))]
    out += [('q = %d' % q, pair(q, 0), {}, kind) for q, kind in ((gap, 1), (gap + 1, 0), (-over, 1), (-over - 1, 0))]
    out += [('q = %d, intron' % q, pair(q, 5000), {}, kind) for q, kind in ((gap, 2), (gap + 1, 0), (-over, 2), (-over - 1, 0))]
    out.append(('other contig', pair(10, 0, contigs=(0, 1)), {}, 0))
    out.append(('a value of exactly 0', pair(10, 5000, scores=(16, 80)), {}, 0))
    out.append(('a value of exactly 1', pair(10, 5000, scores=(17, 80)), {}, 2))
    out.append(('overlap paid once: value 0', pair(-4, 5000, scores=(20, 80)), {}, 0))
    out.append(('overlap paid once: value 1', pair(-4, 5000, scores=(21, 80)), {}, 2))
    return out


def order_case():
    """equal y0: the order is decided by y1, then x0, then the index -> (chains, their ranks)"""
    return [chain(0, 50, 9, 60, 5, 50), chain(0, 50, 9, 60, 5, 40), chain(0, 50, 7, 60, 5, 40), chain(0, 50, 7, 60, 5, 40), chain(0, 50, 3, 60, 4, 90)], [4, 3, 1, 2, 0]


def equal_candidates_case(flip):
    """two predecessors that give chain 2 the same value: the greater rank wins, which is chain 1 (flip: chain 0, whose y0 is the greater)"""
    y0 = (1, 0) if flip else (0, 0)
    return [chain(0, 100, 10, 1000, y0[0], 100), chain(0, 100, 10, 1000, y0[1], 100), chain(0, 50, 1010, 1100, 110, 200)], 0 if flip else 1


def equal_f_case():
    """two paths of equal F on two contigs: the smaller rank is extracted first, and that is chain 1"""
    return [chain(0, 70, 100, 200, 50, 150), chain(1, 70, 100, 200, 40, 150)]


def shared_predecessor_case():
    """A -> B and A -> C with no link between B and C: the second path stops on A, already used, and scores F_C - F_A"""
    return [chain(0, 100, 1000, 1100, 0, 100), chain(0, 90, 1110, 1200, 110, 200), chain(0, 50, 5000, 5100, 112, 190)]


def staircase_case(n=64):
    return [chain(0, 50, 2000 * t, 2000 * t + 100, 150 * t, 150 * t + 100) for t in range(n)]


def isolated_case(n=64):
    return [chain(t, 40 + t % 3, 100, 200, 10, 110) for t in range(n)]


FUZZ_SCORES = (0, 1, 5, 17, 17, 40, 40, 90)


def fuzz_segments(seed, count, most=64, wide=False, scores=FUZZ_SCORES):
    """segments of 0..most chains drawn from small ranges, so that equal keys, equal values and equal F abound (for FUZZ_SMALL); wide: the
    chains are spread far enough for introns and back-splices at the defaults; scores: what a chain's score is drawn from"""
    rng = random.Random(seed)
    out = []
    for s in range(count):
        n = (0, 1, 2, most - 1, most)[s // 10 % 5] if s % 10 == 0 else rng.randint(0, most)
        mine = []
        for _ in range(n):
            x0, y0 = rng.randrange(0, 400000 if wide else 40), rng.randrange(0, 3000 if wide else 24)
            mine.append(chain(rng.randrange(2), rng.choice(scores), x0, x0 + rng.randint(1, 300 if wide else 9), y0,
                              y0 + rng.randint(1, 300 if wide else 9)))
        out.append(mine)
    return out


FUZZ_SMALL = dict(max_query_gap=6, max_overlap=3, max_skew=4, max_intron=12, max_circle=15, intron_cost=3, backsplice_cost=5)
