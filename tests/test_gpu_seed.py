"""K7 on the GPU (csrc/seed.hip): the minimizer index of a resident genome, seeds and chains, every array compared for equality with
the plain statement tests/seed_check.py.  Inputs are seeded and small: genomes of three or four contigs, 15-60 kb in all, reads of
0-1 500 letters.  The sketch's block constants come from the kernel (SeedIndex.info): positions a wave decides per round, positions
of a work item, work items of a workgroup.  Chain parameters at their edges (a gap of exactly max_gap, a skew of exactly max_skew)
are taken from the data: the test first finds, with the checker, the pair of anchors that sits on the edge, and asserts it is there.
Two cases are planted letter by letter and asserted with the checker before the GPU is asked: a branch off a longer chain, whose walk
stops on a used anchor and whose score is the difference (branch_case), and a predecessor exactly 64 anchors back, the last lane of the
chain kernel and the slot of its ring that is overwritten next, against one 65 back (reach_case)."""
import collections
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import seed_check as sc  # noqa: E402
from ciri_long_amd import hip, seed, ssw_wrap  # noqa: E402

pytestmark = pytest.mark.gpu


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


@pytest.fixture(scope='module')
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


class World(object):
    """a genome on the device and as the checker sees it, with its indexes by (k, w, max_occ): each is built once and shared"""

    def __init__(self, ctx, contigs):
        self.contigs, self.text = contigs, dict(contigs)
        self.genome = hip.Genome(ctx, contigs)
        self.check = sc.Genome(contigs)
        self._made = {}

    def index(self, k, w, max_occ=64):
        if (k, w, max_occ) not in self._made:
            self._made[(k, w, max_occ)] = (hip.SeedIndex(self.genome, k=k, w=w, max_occ=max_occ), sc.index(self.check.codes, k, w))
        return self._made[(k, w, max_occ)]

    def close(self):
        for idx, _ in self._made.values():
            idx.close()
        self.genome.close()


def edge_contigs(k, tail):
    """every sketch edge of the issue in one genome of about 17 kb whose last contig ends on a multiple of `tail` bytes"""
    rng = random.Random(100 + k)
    c0 = (dna(rng, 3000) + 'N' + dna(rng, 500) + 'N' * (k - 1) + dna(rng, 500) + 'N' * k + dna(rng, 700) + 'N' * 1500 + dna(rng, 1200) +
          dna(rng, 600).lower() + 'A' * 120 + 'AC' * 80 + 'ACGT' * 6 + 'AATT' * 5 + 'GAATTC' * 3 + dna(rng, 2000))
    c1 = 'ACG'                                          # shorter than every k
    c2 = dna(rng, 5000)                                 # c0's last letters and c2's first must not form a k-mer (c1 holds none)
    c3 = dna(rng, 1111) + 'acgtn' * 7
    total = len(c0) + len(c1) + len(c2) + len(c3)
    c3 += dna(rng, -total % 256)
    if tail == 16:
        c3 += dna(rng, 16)
    assert (len(c0) + len(c1) + len(c2) + len(c3)) % tail == 0 and (tail == 256 or (len(c0) + len(c1) + len(c2) + len(c3)) % 256)
    return [('c0', c0), ('c1', c1), ('c2', c2), ('c3', c3)]


def assert_index(idx, want, max_occ):
    keys, pos, strand = idx.dump()
    got = list(zip(keys.tolist(), pos.tolist(), strand.tolist()))
    assert got == sorted(got)
    assert got == want
    info = idx.info()
    per_key = collections.Counter(key for key, _, _ in want)
    assert (info['entries'], info['distinct'], info['repetitive_keys']) == (len(want), len(per_key), sum(1 for v in per_key.values() if v > max_occ))
    assert info['bytes'] >= 16 * len(want)


@pytest.mark.parametrize('k,w,tail', [(4, 1, 256), (15, 5, 256), (15, 5, 16), (16, 2, 256), (28, 64, 256), (4, 64, 16)])
def test_index_equals_checker(ctx, k, w, tail):
    world = World(ctx, edge_contigs(k, tail))
    try:
        idx, want = world.index(k, w, max_occ=8)
        assert_index(idx, want, 8)
        if k == 16:                                     # ACGT x 4 is its own reverse complement: no entry at its three starts
            at = world.text['c0'].index('ACGT' * 6)
            assert sc.keys(sc.encode('ACGT' * 4), 16) == [None] and not {at, at + 4, at + 8} & {p for _, p, _ in want}
        at = world.text['c0'].index('A' * 120)            # the homopolymer run: every position ties, every position is selected
        if w <= 120 - k + 1:
            assert {p for _, p, _ in want} >= set(range(at + w, at + 120 - k + 1 - w))
    finally:
        world.close()


@pytest.mark.parametrize('k,w', [(15, 5), (4, 64), (28, 1), (16, 2)])
def test_sketch_lengths_and_block_edges(ctx, k, w):
    rng = random.Random(7 * k + w)
    world = World(ctx, [('g', dna(rng, 300))])
    try:
        idx, _ = world.index(k, w)
        info = idx.info()
        rnd, item, block = info['round'], info['item'], info['item'] * info['items_per_block']
        assert (rnd, item, info['items_per_block']) == (64, 1024, 4)
        lengths = [0, k - 1, k, k + w - 2, k + w - 1] + [P + d + k - 1 for P in (rnd, item, block) for d in (-1, 0, 1)]
        seqs = []
        for n in lengths:
            s = [rng.randrange(4) for _ in range(max(n, 0))]
            for _ in range(n // 400):
                a = rng.randrange(n)
                b = min(n, a + rng.choice((1, k - 1, k)))
                s[a:b] = [4] * (b - a)
            seqs.append(np.array(s[:max(n, 0)], dtype=np.int8))
        got = idx.minimizers(seqs)
        for s, (pos, keys, strand) in zip(seqs, got):
            assert list(zip(pos.tolist(), keys.tolist(), strand.tolist())) == sc.sketch(s.tolist(), k, w), len(s)
    finally:
        world.close()


def test_minimizers_of_a_read_equal_the_entries_of_the_same_string_as_a_contig(ctx):
    rng = random.Random(21)
    text = dna(rng, 1500) + 'N' * 20 + dna(rng, 700).lower() + 'T' * 40 + dna(rng, 900)
    world = World(ctx, [('only', text)])
    try:
        idx, want = world.index(15, 5)
        pos, keys, strand = idx.minimizers([text])[0]
        assert sorted(zip(keys.tolist(), pos.tolist(), strand.tolist())) == want and len(want) > 500
    finally:
        world.close()


def test_a_genome_of_n_has_no_entries(ctx):
    world = World(ctx, [('n0', 'N' * 3000), ('n1', 'n' * 100), ('n2', '')])
    try:
        idx, want = world.index(15, 5)
        assert want == [] and idx.info()['entries'] == 0 and len(idx.dump()[0]) == 0
        got = idx.seeds(['ACGTTGCAAGGCTTAGCATCGGATCGATTAGC'])
        assert got['anchor_off'].tolist() == [0, 0] and len(got['x']) == 0
        assert idx.chains(['ACGTTGCAAGGCTTAGCATCGGATCGATTAGC'])[0] == [[]]
    finally:
        world.close()


MAX_OCC = 4


@pytest.fixture(scope='module')
def seed_world(ctx):
    rng = random.Random(31)
    at_most, too_many = dna(rng, 60), dna(rng, 60)
    c0 = ''
    for t in range(MAX_OCC + 1):
        c0 += dna(rng, 700) + (at_most if t < MAX_OCC else '') + dna(rng, 300) + too_many
    world = World(ctx, [('r0', c0 + dna(rng, 500)), ('r1', dna(rng, 6000)), ('r2', dna(rng, 7000))])
    world.at_most, world.too_many = at_most, too_many
    yield world
    world.close()


def seed_reads(world):
    rng = random.Random(32)
    r0, r1 = world.text['r0'], world.text['r1']
    a, b = r0.index(world.at_most), r0.index(world.too_many)
    return [r1[1000:1800], rc(r1[2000:2700]), dna(rng, 500), r0[a - 100:a + 160], r0[b - 100:b + 160], '', 'ACGTACG', 'N' * 200,
            mutate(rng, r1[3000:4000], 0.1), rc(mutate(rng, world.text['r2'][500:1700], 0.1))]


def assert_seeds(got, world, want_idx, reads, k, w, max_occ):
    off = got['anchor_off'].tolist()
    assert off[0] == 0 and len(off) == len(reads) + 1
    for r, text in enumerate(reads):
        anchors, repetitive = sc.seeds(want_idx, sc.encode(text), k, w, max_occ)
        sl = slice(off[r], off[r + 1])
        assert list(zip(got['minus'][sl].tolist(), got['x'][sl].tolist(), got['y'][sl].tolist())) == anchors, r
        assert got['read'][sl].tolist() == [r] * len(anchors) and int(got['repetitive'][r]) == repetitive, r


def test_seeds_equal_checker(seed_world):
    idx, want = seed_world.index(15, 5, MAX_OCC)
    per_key = collections.Counter(key for key, _, _ in want)
    assert MAX_OCC in per_key.values() and MAX_OCC + 1 in per_key.values()
    reads = seed_reads(seed_world)
    got = idx.seeds(reads)
    assert_seeds(got, seed_world, want, reads, 15, 5, MAX_OCC)
    off, rep = got['anchor_off'].tolist(), got['repetitive'].tolist()
    n = [off[r + 1] - off[r] for r in range(len(reads))]
    assert n[0] > 100 and not got['minus'][off[0]:off[1]].any()              # an interval of the genome: the plus strand
    assert n[1] > 100 and got['minus'][off[1]:off[2]].all()                  # its reverse complement: the minus strand, y in the reversed read
    x, y = got['x'][off[1]:off[2]], got['y'][off[1]:off[2]]
    assert (np.diff(x) > 0).all() and (x - y == x[0] - y[0]).all()
    assert n[5:8] == [0, 0, 0] and rep[5:8] == [0, 0, 0]
    assert rep[3] == 0 and rep[4] > 0 and n[3] > n[4]                        # exactly max_occ entries still seed, max_occ + 1 do not
    assert idx.info()['shares'] == 1


def test_seeds_in_shares_and_refusals(seed_world):
    idx, want = seed_world.index(15, 5, MAX_OCC)
    reads = seed_reads(seed_world)
    whole = idx.seeds(reads)
    off = whole['anchor_off'].tolist()
    most = max(off[r + 1] - off[r] for r in range(len(reads)))
    cut = idx.seeds(reads, workspace_bytes=64 * most)
    assert idx.info()['shares'] > 2
    for name in whole:
        assert (whole[name] == cut[name]).all(), name
    with pytest.raises(hip.ClhError, match=r'\(-4\).*read \d+ alone'):
        idx.seeds(reads, workspace_bytes=64 * (most - 1))
    bad = [np.array([0, 1, 2, 3] * 10, dtype=np.int8), np.array([0, 1, 5, 3] * 10, dtype=np.int8)]
    with pytest.raises(hip.ClhError, match=r'\(-2\).*read 1 '):
        idx.seeds(bad)
    for k, w in ((3, 5), (29, 5), (15, 0), (15, 65)):
        with pytest.raises(hip.ClhError, match=r'clh_seed_index_create'):
            hip.SeedIndex(seed_world.genome, k=k, w=w)


@pytest.fixture(scope='module')
def chain_world(ctx):
    rng = random.Random(41)
    twice = dna(rng, 1200)
    unit = dna(rng, 300)
    c2 = dna(rng, 1000) + twice + dna(rng, 2800) + mutate(rng, twice, 0.03) + dna(rng, 1000)
    c3 = dna(rng, 500) + ''.join(mutate(rng, unit, 0.02) for _ in range(15)) + dna(rng, 500)
    world = World(ctx, [('a', dna(rng, 6000)), ('b', dna(rng, 5000)), ('two', c2), ('rep', c3)])
    world.twice, world.unit = twice, unit
    yield world
    world.close()


def assert_chains(world, k, w, reads, **params):
    idx, want_idx = world.index(k, w)
    got, truncated = idx.chains(reads, **params)
    want = [sc.read_chains(world.check, want_idx, sc.encode(t), k, w, 64, **params) for t in reads]
    for r in range(len(reads)):
        assert got[r] == want[r][0], (r, params)
        assert truncated[r].tolist() == want[r][1], (r, params)
    return want


def test_chains_planted_run_two_loci_and_contig_edge(chain_world):
    rng = random.Random(42)
    a, b = chain_world.text['a'], chain_world.text['b']
    reads = [mutate(rng, a[2000:3000], 0.05), rc(mutate(rng, b[1000:2200], 0.05)), mutate(rng, chain_world.twice, 0.02), a[-400:] + b[:400],
             chain_world.unit + chain_world.unit, dna(rng, 700), '']
    want = assert_chains(chain_world, 15, 5, reads)
    assert len(want[0][0]) == 1 and want[0][0][0]['minus'] == 0 and want[0][0][0]['contig'] == 0 and abs(want[0][0][0]['x_first'] - 2000) < 50
    assert want[1][0][0]['minus'] == 1 and want[1][0][0]['contig'] == 1
    two = want[2][0]
    assert len(two) >= 2 and two[0]['score'] >= two[1]['score'] and {two[0]['contig'], two[1]['contig']} == {2} and abs(two[0]['x_first'] - two[1]['x_first']) > 3000
    edge = want[3][0]                                    # colinear across two contigs adjacent in the concatenation: never one chain
    assert [c['contig'] for c in edge] in ([0, 1], [1, 0]) and all(c['x_end'] <= len(chain_world.text['ab'[c['contig']]]) for c in edge)
    assert want[5][0] == [] and want[6][0] == []
    # the doubled unit against 15 copies: thousands of anchors in a segment and the same x under two y (asserted); its interleaved loci and
    # tied chain ends are held to the checker but not asserted one by one
    anchors, _ = sc.seeds(chain_world.index(15, 5)[1], sc.encode(reads[4]), 15, 5, 64)
    plus = [(x, y) for m, x, y in anchors if m == 0]
    assert len(plus) > 2000 and any(p[0] == q[0] for p, q in zip(plus, plus[1:]))
    for params in (dict(lookback=1), dict(lookback=2), dict(lookback=9, max_chains=8), dict(max_chains=1), dict(max_chains=3, max_attempts=3),
                   dict(max_chains=64, max_attempts=5, min_anchors=4), dict(min_score=25, min_anchors=1, max_chains=16),
                   dict(min_score=10 ** 6), dict(max_gap=0), dict(max_skew=0)):
        assert_chains(chain_world, 15, 5, [reads[4], reads[2], reads[0]], **params)
    want = assert_chains(chain_world, 15, 5, [reads[4]], max_chains=2, max_attempts=2, min_anchors=10 ** 6)
    assert want[0][0] == [] and want[0][1][0] is True                                   # attempts run out with chain ends left: truncated


def test_chain_gap_and_skew_on_the_edge(chain_world):
    rng = random.Random(43)
    read = mutate(rng, chain_world.text['a'][3000:4200], 0.08)
    _, want_idx = chain_world.index(15, 5)
    anchors, _ = sc.seeds(want_idx, sc.encode(read), 15, 5, 64)
    seg = [(x, y) for m, x, y in anchors if m == 0]
    f, p = sc.chains(seg, chain_world.check.contig_of, 15)
    links = [(seg[i][0] - seg[p[i]][0], seg[i][1] - seg[p[i]][1]) for i in range(len(seg)) if p[i] >= 0]
    gap = max(max(dx, dy) for dx, dy in links)
    skew = max(abs(dx - dy) for dx, dy in links)
    assert gap > 15 and skew > 0
    for params in (dict(max_gap=gap), dict(max_gap=gap - 1), dict(max_skew=skew), dict(max_skew=skew - 1)):
        assert_chains(chain_world, 15, 5, [read], **params)
    # the link on the edge is taken at the bound and lost one below it
    f1, p1 = sc.chains(seg, chain_world.check.contig_of, 15, max_gap=gap - 1)
    f2, p2 = sc.chains(seg, chain_world.check.contig_of, 15, max_skew=skew - 1)
    assert (f1, p1) != (f, p) and (f2, p2) != (f, p)
    assert sc.chains(seg, chain_world.check.contig_of, 15, max_gap=gap, max_skew=skew) == (f, p)


@pytest.mark.parametrize('lookback', [1, 2, 64])
def test_chain_lookback_reach(chain_world, lookback):
    """the doubled unit puts every x under two y, so the anchor next to one is no predecessor and the nearest sits exactly 2 back: within
    reach of lookback 2 and out of reach of lookback 1"""
    read = chain_world.unit[:200] + chain_world.unit[:200]
    _, want_idx = chain_world.index(15, 5)
    anchors, _ = sc.seeds(want_idx, sc.encode(read), 15, 5, 64)
    seg = [(x, y) for m, x, y in anchors if m == 0]
    f, p = sc.chains(seg, chain_world.check.contig_of, 15, lookback=lookback)
    reach = [i - p[i] for i in range(len(seg)) if p[i] >= 0]
    assert all(r <= lookback for r in reach)
    if lookback == 2:
        assert max(reach) == 2
    if lookback == 1:
        assert sc.chains(seg, chain_world.check.contig_of, 15, lookback=2) != (f, p)
    assert_chains(chain_world, 15, 5, [read], lookback=lookback)


def plus_segment(contigs, read, k, w):
    """the checker's view of one read on one genome: (sc.Genome, its index, the plus-strand anchors (x, y) in order)"""
    check = sc.Genome(contigs)
    want_idx = sc.index(check.codes, k, w)
    anchors, _ = sc.seeds(want_idx, sc.encode(read), k, w, 64)
    return check, want_idx, [(x, y) for m, x, y in anchors if m == 0]


def branch_case():
    """S T X T' on one contig, T' a second copy of T, and the read S T: the anchors of T on T' sit behind those of T on T, the first of
    them reaches back over T's anchors to the end of S (skew |T| + |X| <= max_skew), and the chain S T takes S first -- so the walk
    from the end of T' stops on a used anchor and the chain's score is the difference"""
    rng = random.Random(61)
    s, t, x = dna(rng, 500), dna(rng, 120), dna(rng, 80)
    return [('one', dna(rng, 300) + s + t + x + t + dna(rng, 300))], s + t


def test_chain_branch_scores_the_difference_and_is_dropped_under_min_score(ctx):
    contigs, read = branch_case()
    check, want_idx, seg = plus_segment(contigs, read, 15, 5)
    f, p = sc.chains(seg, check.contig_of, 15)
    got, _ = sc.extract(seg, f, p, 15, min_score=40)
    assert len(got) == 2
    (score0, _, first0, _), (score1, count1, first1, last1) = got
    assert p[first0] == -1 and score0 == f[got[0][3]]                        # the main chain walks to its start
    stop = p[first1]                                                          # the branch: its walk stopped on an anchor the main chain used
    assert stop >= 0 and first0 <= stop <= got[0][3] and score1 == f[last1] - f[stop] and 40 <= score1 < 100 < f[last1] and count1 >= 3
    assert len(sc.extract(seg, f, p, 15, min_score=100)[0]) == 1             # the difference falls under min_score: dropped, though f(e) is above it
    world = World(ctx, contigs)
    try:
        want = assert_chains(world, 15, 5, [read], min_score=40)
        assert [c['score'] for c in want[0][0]] == [score0, score1]
        want = assert_chains(world, 15, 5, [read], min_score=100)
        assert [c['score'] for c in want[0][0]] == [score0]
        assert_chains(world, 15, 5, [read], min_score=score1)
        assert_chains(world, 15, 5, [read], min_score=score1 + 1)
    finally:
        world.close()


def reach_case(between):
    """the read A B C on the contig A C' B at w = 1 (every position an anchor): C' is a piece of C that gives exactly `between` anchors,
    which sort between the last anchor of A and the first of B and, lying later in the read than B, are no predecessors of B (dy < 0):
    the nearest admissible predecessor of B's first anchor is A's last, between + 1 anchors back"""
    rng = random.Random(62)
    a, b, c = dna(rng, 300), dna(rng, 300), dna(rng, 200)
    piece = c[50:50 + between + 14]

    def other(*letters):                                # a letter that continues none of the read's k-mers across a junction of the contig
        return [ch for ch in 'ACGT' if ch not in letters][0]
    contig = dna(rng, 200) + a + other(c[49], b[0]) + piece + other(c[50 + between + 14], a[-1]) + b + other(c[0]) + dna(rng, 200)
    return [('one', contig)], a + b + c


@pytest.mark.parametrize('between,reached', [(63, True), (64, False), (62, True), (30, True)])
def test_chain_predecessor_exactly_lookback_back_and_one_beyond(ctx, between, reached):
    contigs, read = reach_case(between)
    check, want_idx, seg = plus_segment(contigs, read, 15, 1)
    assert len(seg) == 286 + between + 286
    i = 286 + between                                                         # B's first anchor; seg[285] is A's last, seg[286 : i] are C's
    assert seg[i] == (200 + 300 + 1 + between + 14 + 1, 300) and seg[285] == (200 + 285, 285) and all(y >= 650 for _, y in seg[286:i])
    f, p = sc.chains(seg, check.contig_of, 15, lookback=64)
    reach = [j - p[j] for j in range(len(seg)) if p[j] >= 0]
    if reached:
        assert p[i] == 285 and max(reach) == between + 1 and f[i] > 15
    else:
        assert p[i] == -1 and f[i] == 15 and i - 285 == 65                   # one beyond the reach: no link, B starts a chain of its own
    world = World(ctx, contigs)
    try:
        want = assert_chains(world, 15, 1, [read], lookback=64)
        firsts = sorted(c['y_first'] for c in want[0][0] if c['y_first'] < 600)
        assert firsts == ([0] if reached else [0, 300])
        if between == 63:                                                     # the same anchors under a shorter reach: the link is lost
            assert sc.chains(seg, check.contig_of, 15, lookback=63)[1][i] == -1
            assert_chains(world, 15, 1, [read], lookback=63)
    finally:
        world.close()


def test_chain_segment_sizes(chain_world):
    """with w = 1 every valid position is a minimizer: an interval of P + k - 1 letters of a random contig is a segment of exactly P anchors"""
    a = chain_world.text['a']
    reads = [a[500:500 + P + 14] for P in (1, 2, 63, 64, 65, 129)] + [rc(a[900:900 + 64 + 14])]
    _, want_idx = chain_world.index(15, 1)
    for text, P in zip(reads, (1, 2, 63, 64, 65, 129, 64)):
        assert len(sc.seeds(want_idx, sc.encode(text), 15, 1, 64)[0]) == P
    for params in (dict(), dict(min_score=15, min_anchors=1), dict(lookback=1, min_score=20)):
        assert_chains(chain_world, 15, 1, reads, **params)


def test_chain_refusals(chain_world):
    idx, _ = chain_world.index(15, 5)
    for params in (dict(lookback=0), dict(lookback=65), dict(max_chains=0), dict(max_chains=65), dict(max_attempts=0), dict(max_gap=-1)):
        with pytest.raises(hip.ClhError, match=r'clh_seed_chain_batch failed \(-2\)'):
            idx.chains(['ACGT' * 20], **params)


def test_reads_to_extended_alignments_end_to_end(ctx):
    rng = random.Random(51)
    contigs = [('x%d' % c, dna(rng, 20000)) for c in range(3)]
    world = World(ctx, contigs)
    try:
        idx = seed.index(world.genome)
        want_idx = sc.index(world.check.codes, 15, 5)
        reads, truth = [], []
        for r in range(30):
            name, text = contigs[r % 3]
            L = rng.randint(300, 1500)
            a = rng.randrange(0, len(text) - L)
            read = mutate(rng, text[a:a + L], 0.10)
            reads.append(rc(read) if r & 1 else read)
            truth.append((name, a, a + L, bool(r & 1)))
        want = [sc.map_read(world.check, want_idx, sc.encode(t), 15, 5, 64) for t in reads]
        for r, (name, a, b, minus) in enumerate(truth):     # the generator's part: the checker's best chain finds the planted interval
            top = want[r][0]
            assert (top['contig'], top['minus']) == (name, minus) and top['score'] >= 40 and top['anchors'] >= 3, r
            assert top['ref_start'] >= a - 50 and top['ref_end'] <= b + 50 and top['ref_end'] - top['ref_start'] >= (b - a) // 2, r
        got = seed.map_reads(idx, reads)
        assert got == want
        tops = [g[0] for g in got]
        ext = ssw_wrap.extend_anchors_genome(world.genome, [t['anchor'] for t in tops], [t['minus'] for t in tops], reads)
        for r, (name, a, b, minus) in enumerate(truth):     # this pins the anchor convention of seed.map_reads
            res = ext[r]
            overlap = min(res.genome_end + 1, b) - max(res.genome_begin, a)
            assert res.contig == name and overlap >= (b - a) // 2, (r, res.genome_begin, res.genome_end, a, b)
        idx.close()
    finally:
        world.close()
