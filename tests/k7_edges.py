"""The inputs that tests/test_k7_edges_host.py asserts with the checkers alone (link_check, junction_check, circle_check, seed_check) and
tests/test_gpu_k7_edges.py then asks the GPU about: what the feature tests of the link kernel, K7j and K7c leave out.
Link kernel: negative F, scores, coordinates and costs on the 2^40 bound, a fuzz over both, segment counts around a workgroup.
K7j: planted ties and a low-complexity fuzz in the classes of 2, 4 and 8 rows per lane, windows clipped inside those classes, and the
scoring bound 2^20 - 1 at the full span.  K7c: one read that fills every task slot, the planted reads at other strides, batches across
the 256-thread workgroups with one circle of more than 256 reads, coordinates above 2^16 in a contig-major table, and shares."""
import functools
import random

import circle_cases as ccases
import circle_check as cc
import junction_cases as jcases
import junction_check as jc
import link_cases as lcases
import link_check as lc
import seed_check as sc

K, W, MAX_OCC = ccases.K, ccases.W, ccases.MAX_OCC
TOP = (1 << 40) - 1                                     # the greatest score, coordinate and cost the link kernel admits
dna, rc, chain = jcases.dna, jcases.rc, lcases.chain


# ---- link kernel ---------------------------------------------------------------------------------------------------------------------

def staircase(n, score):
    """lcases.staircase_case with chain t scoring score(t): every chain can follow the one, two and three steps below it across an intron"""
    return [chain(0, score(t), 2000 * t, 2000 * t + 100, 150 * t, 150 * t + 100) for t in range(n)]


def negative_cases():
    """[(label, chains, parameters)]: F below 0 in the DP's butterfly and in the extraction's"""
    out = []
    for n in (2, 63, 64):
        out.append(('all negative %d' % n, staircase(n, lambda t: -1 - 7 * t % 5), {}))
        out.append(('alternating %d' % n, staircase(n, lambda t: 50 if t % 2 == 0 else -120), {}))
    out.append(('negative path', [chain(0, 100, 1000, 1100, 0, 100), chain(0, 90, 1110, 1200, 110, 200), chain(0, -50, 5000, 5100, 112, 190)], {}))
    out.append(('value 1, F below 0', lcases.pair(10, 5000, scores=(17, -80)), {}))
    out.append(('value 1, F 0', lcases.pair(10, 5000, scores=(17, -1)), {}))
    out.append(('value 0, F below 0', lcases.pair(10, 5000, scores=(16, -80)), {}))
    return out


def top_cases():
    """[(label, chains, parameters)]: scores of 2^40 - 1 and 1 - 2^40, coordinates of 2^40 - 1, both costs at 2^40 - 1, F of about 2^46"""
    T = TOP
    a, b = chain(0, T, 1000, 1100, 0, 100), chain(0, T, 1110, 1210, 110, 210)
    out = [('coordinates and scores', [chain(0, T, T - 2200, T - 2100, T - 250, T - 150), chain(0, -T, T - 100, T, T - 100, T)], {}),
           # b follows a with no cost (F 2 T), c follows b across an intron and e follows b across a back-splice, each for all but T of it
           ('costs', [a, b, chain(0, 5, 9000, 9100, 220, 320), chain(0, 7, 500, 600, 330, 430)], dict(intron_cost=T, backsplice_cost=T)),
           ('costs, value 0', [a, chain(0, 5, 9000, 9100, 110, 210), chain(0, 7, 500, 600, 120, 220)], dict(intron_cost=T, backsplice_cost=T)),
           ('staircase of 64', staircase(64, lambda t: T), {}),
           ('mixed', [chain(0, T, 1000, 1100, 0, 100), chain(0, -T, 1110, 1200, 110, 200), chain(0, 3, 5000, 5100, 210, 300), chain(1, -1, 10, 20, 5, 15)], {})]
    return out


RANGE_SCORES = (-TOP, 1 - TOP, -1000, -17, -1, 0, 0, 1, 5, 17, 40, 90, TOP - 1, TOP)


def range_fuzz():
    """[(segments, parameters)]: lcases.fuzz_segments with the scores drawn from negative, zero, small and near-bound values"""
    return [(lcases.fuzz_segments(21, 100, scores=RANGE_SCORES), lcases.FUZZ_SMALL), (lcases.fuzz_segments(22, 40, wide=True, scores=RANGE_SCORES), {})]


def workgroup_segments(nseg):
    """nseg segments, the last one full (64 chains): a workgroup takes 4 of them"""
    pool = [mine for _, mine, p in negative_cases() + top_cases() if not p]
    return [pool[(3 * s) % len(pool)] for s in range(nseg - 1)] + [staircase(64, lambda t: 40 + 9 * t % 7 - (60 if t % 5 == 0 else 0))]


# ---- K7j -----------------------------------------------------------------------------------------------------------------------------
# A batch is junction_cases': (contigs [(name, text)], reads [text], tasks [(read, minus, contig, xd, yd, xa, ya, strand)], scoring)

CLASS_SPANS = ((1, 35), (2, 70), (3, 150))              # (class, a): the anchors stand `a` letters either side of the shared letters, m = 2 a + slide


def slide_batches():
    """jcases.slide_cases with the anchors moved apart until m lands in class 1, 2 and 3: one batch per class, every slide of 1, 2 and 3
    letters on the plus read and on its reverse complement as a minus read, want in {0, +1, -1}
    -> [(class, [(slide, a, want)] per task, batch)]; the tie is t = a .. a + slide on every strand asked for, and its first t is a"""
    out = []
    for cls, a in CLASS_SPANS:
        contigs, texts, tasks, planted = [], [], [], []
        for slide in (1, 2, 3):
            rng = random.Random(400 + 10 * cls + slide)
            shared = 'ACG'[:slide]
            X, Y = dna(rng, a + 30) + 'T', 'T' + dna(rng, a + 30)
            head = dna(rng, 30) + 'A'
            body = head + shared + Y + dna(rng, 200) + X + shared + 'A' + dna(rng, 30)
            xa_core = len(head)                                               # where shared + Y begins
            xd_core = len(head) + slide + len(Y) + 200 + len(X)               # where shared begins behind X
            yd, ya = len(X) - a, len(X) + slide + a
            c = len(contigs)
            contigs.append(('h%d' % slide, body))
            texts += [X + shared + Y, rc(X + shared + Y)]
            for minus in (0, 1):
                for want in (0, 1, -1):
                    tasks.append((2 * c + minus, minus, c, xd_core - a, yd, xa_core + slide + a, ya, want))
                    planted.append((slide, a, want))
        out.append((cls, planted, (contigs, texts, tasks, dict(slack=4, noncanonical=6, donor_costs={'GT': 6}, acceptor_costs={'AG': 6}))))
    return out


def class_fuzz_batches(seed=12, per_class=8):
    """jcases.fuzz_batches' letters (A four times as likely as C) at m drawn from each of the classes 1, 2 and 3: per_class tasks of
    every class in one batch per slack of 0, 5 and 64"""
    rng = random.Random(seed)
    contigs = [('w%d' % c, dna(rng, rng.randint(150, 900), 'AAAAC')) for c in range(4)]
    texts = [dna(rng, rng.randint(520, 700), 'AAAAC') for _ in range(6)]
    out = []
    for slack in (0, 5, 64):
        tasks = []
        for n in range(3 * per_class):
            lo, hi = ((65, 128), (129, 256), (257, 512))[n % 3]
            r, c = rng.randrange(len(texts)), rng.randrange(len(contigs))
            m = rng.choice((lo, hi, rng.randint(lo, hi), rng.randint(lo, hi)))
            yd = rng.randint(0, len(texts[r]) - m)
            size = len(contigs[c][1])
            xa = rng.randint(0, size - 1)
            tasks.append((r, rng.randrange(2), c, rng.randint(xa + 1, size), yd, xa, yd + m, 0))
        out.append((contigs, texts, tasks, dict(slack=slack)))
    return out


CLIPS = (63, 64, 65, 128, 129)


def clip_batch():
    """windows clipped inside classes 1-3 on a contig of 300 letters between two neighbours: nD = 0 and nA = 0 at m of 65, 130, 300 and
    512, and nD, nA of 63, 64, 65, 128 and 129, below m, so that the 64-column fetch loop ends where the contig does; N in the contig,
    code 4 in the reads, minus reads, every strand asked for"""
    rng = random.Random(78)
    mid = dna(rng, 150) + 'N' + dna(rng, 149)
    contigs = [('left', dna(rng, 60) + 'AG'), ('mid', mid), ('right', 'GT' + dna(rng, 60))]
    size = len(mid)
    fwd = dna(rng, 20) + mid[40:] + mid[:260] + dna(rng, 20)
    fwd = fwd[:100] + 'N' + fwd[101:]
    texts = [fwd, rc(dna(rng, 15) + mid[30:] + 'N' + mid[:270] + dna(rng, 14)), dna(rng, 600)]
    assert min(len(t) for t in texts) >= 520
    places = [(size, 0, m) for m in (65, 130, 300, 512)]
    for n in CLIPS:
        m = min(v for v in (70, 140, 300) if v > n)
        places += [(size - n, n, m), (size - n, n, 512), (size, n, m), (size - n, 0, m)]
    tasks = []
    for i, (xd, xa, m) in enumerate(places):
        r = i % 3
        minus = 1 if r == 1 else (i // 3) % 2
        tasks.append((r, minus, 1, xd, (len(texts[r]) - m) // 2 if i % 2 else 0, xa, ((len(texts[r]) - m) // 2 if i % 2 else 0) + m, (0, 1, -1)[(i // 3 + i) % 3]))
    return contigs, texts, tasks, dict(slack=16)


# (2 * 512 + 64) * 963 + 500 + 165 + 166 = 2^20 - 1: the bound of seed_device.h at the full span and the full slack
BOUND_SCORING = dict(max_span=512, slack=64, match=963, mismatch=962, gap_open=963, gap_extend=950, intron_open=500, noncanonical=165,
                     donor_costs={'GT': 0}, acceptor_costs={'AG': 0, 'AC': 166})
BOUND_SPANS = (1, 64, 65, 511, 512)


def bound_planted(spans=BOUND_SPANS, seed=51):
    """planted junctions (jcases.spliced_task, 5 % noise above 8 letters) under BOUND_SCORING"""
    rng = random.Random(seed)
    contigs, texts, tasks = [], [], []
    for n, m in enumerate(spans):
        body, text, task = jcases.spliced_task(rng, m, noise=0.05 if m > 8 else 0.0, minus=n & 1, strand=(0, 1, -1)[n % 3])
        contigs.append(('b%d' % n, body))
        texts.append(text)
        tasks.append((n, task[0], n) + task[1:])
    return contigs, texts, tasks, dict(BOUND_SCORING)


def bound_batches():
    """m of 1, 64, 65, 511 and 512 under BOUND_SCORING three ways -> {'planted', 'unrelated', 'poly'}: planted junctions; a read that has
    nothing to do with its contig; a poly-A read against poly-C windows, where every cell is a mismatch or a gap and the keys are the
    most negative that can be"""
    rng = random.Random(52)
    body = dna(rng, 2400)
    texts = [dna(rng, 600), dna(rng, 560)]
    unrelated = [(n & 1, n & 1, 0, 1500, 10, 800, 10 + m, (0, 1, -1)[n % 3]) for n, m in enumerate(BOUND_SPANS)]
    poly = 'C' * 700 + dna(rng, 100) + 'C' * 700
    both = [(0, n & 1, 0, 800, 0, 700, m, (0, -1, 1)[n % 3]) for n, m in enumerate(BOUND_SPANS)]
    return {'planted': bound_planted(), 'unrelated': ([('u', body)], texts, unrelated, dict(BOUND_SCORING)),
            'poly': ([('p', poly)], ['A' * 560], both, dict(BOUND_SCORING))}


# ---- K7c -----------------------------------------------------------------------------------------------------------------------------
FULL = dict(max_skew=100, min_score=30, max_chains=64, max_query_gap=600)
FULL_JUNK = {6: 70, 18: 140, 30: 300, 42: 520}         # letters of junk behind the 6th, 18th, 30th and 42nd piece of the full read


@functools.lru_cache(maxsize=None)
def full_world():
    """-> (contigs, the full read): ccases' contigs and behind them `full`, 200 + 64 * 130 + 200 random letters; the read is its 64
    pieces of 90 letters, taken 130 apart, in DESCENDING order, so that every piece follows the one before it across a back-splice"""
    rng = random.Random(5)
    text = dna(rng, 200 + 64 * 130 + 200)
    read = ''
    for n, piece in enumerate(reversed(range(64)), 1):
        read += text[200 + 130 * piece:200 + 130 * piece + 90]
        if n in FULL_JUNK:
            read += dna(rng, FULL_JUNK[n])
    return list(ccases.world()[0]) + [('full', text)], read


@functools.lru_cache(maxsize=None)
def full_texts():
    """ccases' reads, then the full read and its reverse complement"""
    read = full_world()[1]
    return tuple(ccases.texts()) + (read, rc(read))


FULL_READ = len(ccases.reads())                         # the full read's place in full_texts()


@functools.lru_cache(maxsize=None)
def full_indexed():
    genome = sc.Genome(full_world()[0])
    return genome, sc.index(genome.codes, K, W)


@functools.lru_cache(maxsize=None)
def full_segments(text, max_chains):
    genome, idx = full_indexed()
    chain_p, _, _ = cc.split(dict(FULL, max_chains=max_chains))
    return lc.segment_chains(genome, idx, sc.encode(text), K, W, MAX_OCC, **chain_p)


@functools.lru_cache(maxsize=None)
def full_row(text, max_chains=16):
    """the circle row of one read of the full world at FULL but for max_chains (FULL is ccases.LINK but for it); no word of a row
    depends on the read's place in its batch"""
    genome, _ = full_indexed()
    _, link_p, junction_p = cc.split(dict(FULL, max_chains=max_chains))
    return cc.row(genome, sc.encode(text), 0, full_segments(text, max_chains), K, 0, link_p, junction_p)


def full_tasks(text, max_chains):
    """-> (segments, best path, its K7j tasks, their rows) of a read of the full world"""
    genome, _ = full_indexed()
    _, link_p, junction_p = cc.split(dict(FULL, max_chains=max_chains))
    segs = full_segments(text, max_chains)
    best = cc.best_path(segs, K, 0, **link_p)
    mine = cc.tasks(0, best[0], segs[best[0]], best[2], best[3], K) if best else []
    return segs, best, mine, [jc.refine(genome.codes[t[2]], sc.encode(text), (t[1],) + tuple(t[3:]), **junction_p) for t in mine]


def expected(texts, max_chains=16):
    """(rows, circle_of_read, table) of a batch of the full world, from the cached rows of its reads"""
    rows = [full_row(t, max_chains) for t in texts]
    tab, where = cc.table(rows)
    return rows, where, tab


def middle_batch():
    """the full read in the middle of a few planted ones"""
    texts = full_texts()
    return [texts[r] for r in (0, ccases.label('linear'), 7, FULL_READ, ccases.label('too wide'), 12, ccases.label('empty'))]


HUB = 'plus transcript'                                 # the read whose circle the hub batch holds more than 256 times


@functools.lru_cache(maxsize=None)
def by_status():
    """{status: the reads of full_texts() that have it}, at max_chains 16"""
    out = {s: [] for s in range(4)}
    for r, t in enumerate(full_texts()):
        out[full_row(t)[0]].append(r)
    return out


def hub_reads():
    """the reads that name the hub's circle"""
    texts = full_texts()
    key = full_row(texts[ccases.label(HUB)])[1:5]
    return [r for r in by_status()[0] if full_row(texts[r])[1:5] == key]


@functools.lru_cache(maxsize=None)
def cycled(n, hub=False, last=None):
    """-> the reads (places in full_texts()) of a batch of n: the reads with a circle in a shuffled order, behind every one of them one
    without, of status 1, 2, 3 in turn; hub: every second read names the hub's circle instead, and the rest cycles 1, 2, 3, a circle;
    last: 'found' / 'none' puts a read with / without a circle at the end"""
    by = by_status()
    found = list(by[0])
    random.Random(80 + n).shuffle(found)
    hubs = hub_reads()
    out, at = [], 0
    while len(out) < n:
        if hub:
            out.append(hubs[(at * at) % len(hubs)])
            out.append(found[(at // 4) % len(found)] if at % 4 == 3 else by[1 + at % 4][(at // 4) % len(by[1 + at % 4])])
        else:
            out += [found[at % len(found)], by[1 + at % 3][(at // 3) % len(by[1 + at % 3])]]
        at += 1
    out = out[:n]
    if last == 'found':
        out[-1] = found[0]
    if last == 'none':
        out[-1] = by[2][0]
    return tuple(out)


BATCHES = ((255, False, None), (256, False, 'found'), (256, False, 'none'), (257, False, None), (513, True, None))


def share_batch():
    """the full read between stretches of planted reads that have anchors: cut at its own anchors, it is a share alone"""
    by = by_status()
    some = [r for r in by[0] + by[2] if r != FULL_READ and r != FULL_READ + 1]
    return tuple(some[:9] + [FULL_READ] + some[9:18])


def greedy_shares(anchor_off, cap):
    """the shares of whole reads the library cuts at `cap` anchors: [(first read, behind the last)]"""
    out, a, n = [], 0, len(anchor_off) - 1
    while a < n:
        b = a
        while b < n and anchor_off[b + 1] - anchor_off[a] <= cap:
            b += 1
        assert b > a
        out.append((a, b))
        a = b
    return out


# a world of its own for coordinates above 2^16: `far` (about 70 kb) holds two one-exon circles that share a start beyond 65 536 and differ
# in their end; `near` a circle; `low` a circle that starts below 256.  The table is contig-major, whatever the starts.
@functools.lru_cache(maxsize=None)
def far_world():
    """-> (contigs, circles {label: (contig index, start, end)}, reads [(label of its circle or None, text)])"""
    rng = random.Random(71)
    exon = ccases.exon
    contigs, circles = [], {}
    head = dna(rng, 66000) + 'AG'
    short = exon(rng, 260)
    longer = short + 'GT' + dna(rng, 197) + 'A'          # the short circle's donor is inside the long one
    contigs.append(('far', head + longer + 'GT' + dna(rng, 3000)))
    circles['short'] = (0, len(head), len(head) + len(short))
    circles['long'] = (0, len(head), len(head) + len(longer))
    for c, (name, lead) in enumerate((('near', 300), ('low', 100)), 1):
        front = dna(rng, lead) + 'AG'
        body = exon(rng, 240 + 10 * c)
        contigs.append((name, front + body + 'GT' + dna(rng, 250)))
        circles[name] = (c, len(front), len(front) + len(body))
    assert sum(len(t) for _, t in contigs) <= 80000

    def turn(label, cut):
        c, a, b = circles[label]
        body = contigs[c][1][a:b]
        return body[cut:] + body[:cut]
    reads = [('low', turn('low', 120)), ('long', turn('long', 330)), ('near', rc(turn('near', 100))), ('short', rc(turn('short', 130))), (None, dna(rng, 300)),
             ('long', rc(turn('long', 150))), ('short', turn('short', 100)), ('low', rc(turn('low', 90))), ('near', turn('near', 140)), ('short', turn('short', 160)),
             (None, contigs[0][1][20000:20400])]
    return contigs, circles, reads


@functools.lru_cache(maxsize=None)
def far_want():
    """-> (sc.Genome, (rows, circle_of_read, table)) of the far world's reads at ccases.LINK by the checker"""
    contigs, _, reads = far_world()
    genome = sc.Genome(contigs)
    idx = sc.index(genome.codes, K, W)
    return genome, cc.circles(genome, idx, [sc.encode(t) for _, t in reads], K, W, MAX_OCC, **dict(ccases.LINK))
