"""The planted inputs that tests/test_junction_host.py asserts with the checker alone (tests/junction_check.py) and
tests/test_gpu_junction.py then asks the GPU about: a world of its own -- contigs of at most 4 kb with one gene of 4-6 exons each, circles
made of interior exons only (so both flanks are GT..AG, CT..AC for a gene on '-'), reads that are one copy of a circle, rotated, on either
strand, error-free and with 8 % errors -- and planted tasks: sizes around the class bounds, clipped windows, a neighbouring contig that
begins with the canonical dinucleotide, code 4, soft-masked letters, slides of 1-3 letters, and a seeded fuzz over the letters A, C."""
import functools
import random

import junction_check as jc
import link_check as lc
import seed_check as sc

K, W, MAX_OCC = 15, 5, 64
# introns of 150-400 letters: the chain's and the link's max_skew must lie below them, a circle's span above it
LINK = dict(max_skew=100, min_score=30, max_chains=16)


def dna(rng, n, letters='ACGT'):
    return ''.join(rng.choice(letters) for _ in range(n))


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


def gene(rng, strand):
    """-> (text, exons [(start, end)], end exclusive): 4-6 exons of 130-220 letters that begin and end with A or T, so that no junction can
    slide along a shared letter, introns of 150-400 letters that read GT..AG on the gene's strand (CT..AC on the contig for '-')"""
    text, exons = '', []
    for e in range(rng.randint(4, 6)):
        if e:
            inner = dna(rng, rng.randint(150, 400) - 4)
            text += ('GT' + inner + 'AG') if strand == '+' else ('CT' + inner + 'AC')
        ln = rng.randint(130, 220)
        exons.append((len(text), len(text) + ln))
        text += rng.choice('AT') + dna(rng, ln - 2) + rng.choice('AT')
    return text, exons


@functools.lru_cache(maxsize=None)
def world(seed=23):
    """-> (contigs [(name, text)], genes [(contig, strand, exons in contig coordinates)]): four contigs of at most 4 kb, a gene each"""
    rng = random.Random(seed)
    contigs, genes = [], []
    for c in range(4):
        strand = '+-'[c & 1]
        head = dna(rng, 200)
        body, exons = gene(rng, strand)
        genes.append(('j%d' % c, strand, [(len(head) + a, len(head) + b) for a, b in exons]))
        contigs.append(('j%d' % c, head + body + dna(rng, 200)))
    assert max(len(t) for _, t in contigs) <= 4096
    return contigs, genes


@functools.lru_cache(maxsize=None)
def reads(seed=23):
    """-> [dict]: text, minus (the read's strand), errors, gene, contig, strand (the gene's), exons (the circle's, ascending), circle (start,
    end) 0-based and exclusive, cut (the offset inside the circle at which the read begins), first (the exon the read begins in) and split
    (True where the rotation cuts that exon)"""
    contigs, genes = world(seed)
    text_of = dict(contigs)
    rng = random.Random(seed + 1)
    out = []
    for gi, (name, strand, exons) in enumerate(genes):
        ctg = text_of[name]
        for variant in range(6):
            a = rng.randrange(1, len(exons) - 1)
            b = rng.randrange(a, len(exons) - 1)
            if variant == 3 and a == b:                 # the rotation on an exon boundary needs two exons
                a, b = 1, 2
            mine = exons[a:b + 1]
            circ = ''.join(ctg[e0:e1] for e0, e1 in mine)
            if variant == 3:
                cut, first, split = mine[0][1] - mine[0][0], 1, False
            else:
                cut = rng.randint(60, len(circ) - 60)
                at, first = 0, 0
                while at + (mine[first][1] - mine[first][0]) <= cut:
                    at += mine[first][1] - mine[first][0]
                    first += 1
                split = cut != at
            text = circ[cut:] + circ[:cut]
            errors = variant >= 4
            if errors:
                text = mutate(rng, text, 0.08)
            minus = bool((gi + variant) & 1)
            out.append({'text': rc(text) if minus else text, 'minus': minus, 'errors': errors, 'gene': gi, 'contig': name, 'strand': strand, 'exons': mine,
                        'circle': (mine[0][0], mine[-1][1]), 'cut': cut, 'first': first, 'split': split})
    return out


@functools.lru_cache(maxsize=None)
def checked(seed=23):
    """-> (sc.Genome, its index, per read the checker's link_reads paths): the checker's view, computed once"""
    contigs, _ = world(seed)
    genome = sc.Genome(contigs)
    idx = sc.index(genome.codes, K, W)
    return genome, idx, [lc.link_read(genome, idx, sc.encode(r['text']), K, W, MAX_OCC, **dict(LINK)) for r in reads(seed)]


@functools.lru_cache(maxsize=None)
def refined(seed=23):
    """-> per read the checker's refine_junctions paths at the default scoring"""
    genome, _, paths = checked(seed)
    return [jc.refine_paths(genome, sc.encode(r['text']), mine, K) for r, mine in zip(reads(seed), paths)]


def expected_exons(read):
    """for an error-free read: per piece of map_spliced(refine=True) the planted exons it holds, (start, end) inclusive; the cut ends of a
    split exon are open (None)"""
    mine = [(a, b - 1) for a, b in read['exons']]
    f = read['first']
    if not read['split']:
        return [mine[f:], mine[:f]]
    return [[(None, mine[f][1])] + mine[f + 1:], mine[:f] + [(mine[f][0], None)]]


# ---- planted tasks -------------------------------------------------------------------------------------------------------------------
# A batch is (contigs [(name, text)], reads [text], tasks [(read, minus, contig, xd, yd, xa, ya, strand)], scoring)

def spliced_task(rng, m, noise=0.0, contig_len=2400, strand=0, minus=0):
    """one contig and one read whose m letters between the anchors cross a planted back-splice: the read leaves the contig at `end` and
    re-enters at `start`, GT behind the one and AG in front of the other; -> (contig text, read text, task without read and contig)"""
    t = rng.randint(0, m)
    start, end = rng.randint(20, 200), contig_len - rng.randint(20, 200)
    body = list(dna(rng, contig_len))
    body[end:end + 2] = 'GT'
    body[start - 2:start] = 'AG'
    body = ''.join(body)
    lead, tail = rng.randint(0, 30), rng.randint(0, 30)
    piece = body[end - t - lead:end] + body[start:start + (m - t) + tail]
    if noise:
        piece = piece[:lead] + mutate(rng, piece[lead:lead + m], noise)[:m].ljust(m, 'A') + piece[lead + m:]
    text = rc(piece) if minus else piece
    return body, text, (minus, end - t, lead, start + (m - t), lead + m, strand)


def size_batches(bounds, max_span):
    """tasks with m around every class bound, at slack 0, 16 and 64, in one batch per slack: 1, 2, and every bound - 1, bound, bound + 1 up
    to max_span; beside them one task of m = max_span + 1 (status 1) and two whose anchors cross (status 2)"""
    sizes = sorted({1, 2} | {b + d for b in bounds for d in (-1, 0, 1) if b + d <= max_span})
    out = []
    for slack in (0, 16, 64):
        rng = random.Random(100 + slack)
        contigs, texts, tasks = [], [], []
        for m in sizes + [max_span + 1]:
            body, text, task = spliced_task(rng, m, noise=0.05 if m > 8 else 0.0, minus=len(tasks) & 1, strand=(0, 1, -1)[len(tasks) % 3])
            contigs.append(('s%d' % len(contigs), body))
            texts.append(text)
            tasks.append((len(texts) - 1, task[0], len(contigs) - 1) + task[1:])
        r, minus, c, xd, yd, xa, ya, s = tasks[3]
        tasks.insert(2, (r, minus, c, xa, yd, xa, ya, s))            # xa == xd: crossing
        tasks.insert(7, (r, minus, c, xd, ya, xa, ya, s))            # m == 0
        out.append((contigs, texts, tasks, dict(slack=slack, max_span=max_span)))
    return out


def routing_batch(bounds, waves, seed=5):
    """more tasks of every class than one workgroup holds, the classes interleaved and unordered, the strands mixed, many tasks on one read"""
    rng = random.Random(seed)
    contigs, texts, tasks = [], [], []
    for n in range(3 * waves * len(bounds) + 3):
        lo = 1 if n % len(bounds) == 0 else bounds[n % len(bounds) - 1] + 1
        m = rng.randint(lo, min(bounds[n % len(bounds)], lo + 40))
        body, text, task = spliced_task(rng, m, noise=0.04, contig_len=1200, minus=rng.randrange(2), strand=rng.choice((0, 0, 1, -1)))
        contigs.append(('r%d' % n, body))
        texts.append(text)
        tasks.append((n, task[0], n) + task[1:])
    long_read = dna(rng, 700)
    texts.append(long_read)
    for n in range(40):                                 # many tasks on one read, anywhere on any contig
        yd = rng.randint(0, 600)
        m = rng.randint(1, 90)
        c = rng.randrange(len(contigs))
        xa = rng.randint(0, 1100)
        tasks.append((len(texts) - 1, n & 1, c, rng.randint(xa + 1, 1200), yd, xa, yd + m, rng.choice((0, 1, -1))))
    rng.shuffle(tasks)
    return contigs, texts, tasks, dict(slack=16)


def window_batch():
    """windows clipped at both contig ends down to nD = 0 and nA = 0; a neighbouring contig that begins with GT and one that ends with AG,
    which must cost `other`, not 0; code 4 in the read; N and lower-case letters in the genome; minus reads"""
    rng = random.Random(77)
    mid = dna(rng, 120)
    contigs = [('left', dna(rng, 60) + 'AG'), ('mid', mid), ('right', 'GT' + dna(rng, 60)),
               ('soft', (dna(rng, 40) + 'NN' + dna(rng, 40)).lower() + dna(rng, 38) + 'N' + 'gt' + dna(rng, 40))]
    texts = [mid[100:120] + mid[0:20], rc(mid[90:120] + mid[0:25]), dna(rng, 50), 'ACGTNNACGTAC' + mid[110:120] + 'N' + mid[0:9] + 'NACGT']
    tasks = []
    for strand in (0, 1, -1):
        tasks += [(0, 0, 1, 120, 20, 0, 20 + m, strand) for m in (1, 5, 20)]                   # xd == len: nD = 0; xa == 0: nA = 0
        tasks += [(0, 0, 1, 110, 10, 12, 32, strand), (0, 0, 1, 118, 18, 3, 23, strand), (0, 0, 1, 119, 0, 1, 40, strand)]
        tasks += [(1, 1, 1, 110, 20, 12, 42, strand), (1, 1, 1, 120, 30, 0, 31, strand), (1, 0, 1, 110, 20, 12, 42, strand)]
        tasks += [(3, 0, 1, 115, 17, 5, 28, strand), (3, 1, 1, 115, 0, 5, 37, strand), (3, 0, 1, 120, 0, 0, 37, strand)]
        tasks += [(2, 0, 3, 121, 5, 30, 35, strand), (2, 1, 3, 125, 0, 44, 50, strand), (2, 0, 3, 163, 3, 80, 43, strand)]
        tasks += [(2, 0, 0, 62, 5, 0, 20, strand), (2, 0, 2, 62, 5, 0, 20, strand), (2, 1, 0, 61, 0, 1, 8, strand)]
    return contigs, texts, tasks, dict(slack=16)


def slide_cases():
    """planted homology: the read holds X + shared + Y once; on the contig X + shared stands in front of the donor end and shared + Y
    behind the acceptor start, shared of 1, 2 or 3 letters, and every site costs the same, so the junction can stand at shared + 1
    places and nowhere else (X ends and Y begins with T, the contig goes on with A behind X + shared and has A in front of shared + Y);
    -> [(slide, first t of the tie, batch)], each batch one task over an error-free read"""
    out = []
    for slide in (1, 2, 3):
        rng = random.Random(300 + slide)
        shared = 'ACG'[:slide]
        X, Y = dna(rng, 40) + 'T', 'T' + dna(rng, 40)
        head = dna(rng, 30) + 'A'
        body = head + shared + Y + dna(rng, 200) + X + shared + 'A' + dna(rng, 30)
        xa_core = len(head)                                               # where shared + Y begins
        xd_core = len(head) + slide + len(Y) + 200 + len(X)               # where shared begins behind X
        yd, ya = len(X) - 10, len(X) + slide + 10
        task = (0, 0, 0, xd_core - 10, yd, xa_core + slide + 10, ya, 0)
        out.append((slide, 10, ([('h', body)], [X + shared + Y], [task], dict(slack=4, noncanonical=6, donor_costs={'GT': 6}, acceptor_costs={'AG': 6}))))
    return out


def fuzz_batches(seed=11, count=300):
    """`count` tasks with m <= 14 over the letters A, C alone (A four times as likely as C: on strand - the dinucleotide AC is a free site,
    and with C rare enough a good share of the tasks has no use for one, so that both strands tie), a third each at slack 0, 2 and 5"""
    rng = random.Random(seed)
    contigs = [('f%d' % c, dna(rng, rng.randint(30, 90), 'AAAAC')) for c in range(4)]
    texts = [dna(rng, rng.randint(14, 40), 'AAAAC') for _ in range(24)]
    out = []
    for slack in (0, 2, 5):
        tasks = []
        for _ in range(count // 3):
            r, c = rng.randrange(len(texts)), rng.randrange(len(contigs))
            m = rng.randint(1, 14)
            yd = rng.randint(0, len(texts[r]) - m)
            size = len(contigs[c][1])
            xa = rng.randint(0, size - 1)
            tasks.append((r, rng.randrange(2), c, rng.randint(xa + 1, size), yd, xa, yd + m, 0))
        out.append((contigs, texts, tasks, dict(slack=slack)))
    return out


def score_batches():
    """the scoring edges over one planted batch: gap_open == gap_extend, gap_extend = 0, match = 0, custom tables, costs just under the bound"""
    rng = random.Random(41)
    contigs, texts, tasks = [], [], []
    for n, m in enumerate((3, 17, 40, 64, 65, 100)):
        body, text, task = spliced_task(rng, m, noise=0.1, contig_len=900, minus=n & 1)
        contigs.append(('c%d' % n, body))
        texts.append(text)
        tasks.append((n, task[0], n) + task[1:])
    scorings = [dict(gap_open=2, gap_extend=2), dict(gap_extend=0), dict(match=0), dict(match=0, mismatch=0, gap_open=0, gap_extend=0, intron_open=0, noncanonical=0),
                dict(donor_costs={'GT': 3, 'GC': 1, 'AT': 0}, acceptor_costs={'AG': 2, 'AC': 0}, noncanonical=9, intron_open=0),
                # (2 * 100 + 16) * 4800 + 10000 + 887 + 888 = 2^20 - 1
                dict(max_span=100, slack=16, match=4800, mismatch=4799, gap_open=4800, gap_extend=4700, intron_open=10000, noncanonical=887,
                     donor_costs={'GT': 0}, acceptor_costs={'AG': 0, 'AC': 888})]
    p = jc.parameters(scorings[-1])
    donor, acceptor, other = jc.tables(p)
    assert (2 * 100 + 16) * 4800 + 10000 + max(donor + [other]) + max(acceptor + [other]) == jc.BOUND - 1 and jc.admitted(p) is None
    return [(contigs, texts, tasks, s) for s in scorings]


def codes_of(batch):
    """a batch as the checker takes it: (contigs as code lists, reads as code lists)"""
    return [sc.encode(t) for _, t in batch[0]], [sc.encode(t) for t in batch[1]]


def want_rows(batch):
    """the checker's rows of a batch"""
    contigs, texts = codes_of(batch)
    return [jc.refine(contigs[t[2]], texts[t[0]], (t[1],) + tuple(t[3:]), **batch[3]) for t in batch[2]]
