"""K7's link step on the GPU (csrc/seed_link.hip): the chains of a (read, strand) segment linked into paths across introns and
back-splice junctions, every array compared for equality with the plain statement tests/link_check.py.  The planted rows and the
planted genomes are those of tests/link_cases.py, which tests/test_link_host.py asserts with the checker alone: segment sizes around the
wave (0, 1, 2, 63, 64 chains), every threshold on and one beside its bound, the tie rules, the path shapes, a seeded fuzz drawn from
small ranges, every refusal, and reads that are one copy of a circle, rotated, through links / link_reads / link_chains / map_spliced."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import link_cases as cases  # noqa: E402
import link_check as lc  # noqa: E402
import seed_check as sc  # noqa: E402
from ciri_long_amd import hip, seed, ssw_wrap  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def world(ctx):
    """the planted genome on the device with its index at k = 15, w = 5, and the checker's view of it"""
    contigs, _ = cases.world()
    genome = hip.Genome(ctx, contigs)
    idx = seed.index(genome, k=cases.K, w=cases.W, max_occ=cases.MAX_OCC)
    yield idx
    idx.close()
    genome.close()


def planted(segments, max_chains=None):
    """chain lists -> (counts, rows) as SeedIndex.link_rows takes them; the rows behind a segment's count keep the marker of no chain"""
    most = max([len(s) for s in segments] + [1]) if max_chains is None else max_chains
    rows = np.full((len(segments), most, 10), -7, dtype=np.int64)
    for s, mine in enumerate(segments):
        for c, v in enumerate(mine):
            rows[s, c] = (s >> 1, v['minus'], v['contig'], v['score'], v['anchors'], v['x_first'], v['y_first'], v['x_end'], v['y_end'], 0)
    return np.array([len(s) for s in segments], dtype=np.int64), rows


def assert_rows(idx, segments, max_chains=None, **p):
    counts, rows = planted(segments, max_chains)
    got = idx.link_rows(counts, rows, **p)
    assert got['link_rows'].shape == (len(segments), rows.shape[1], 8)
    for s, mine in enumerate(segments):
        want, paths = lc.rows(mine, idx.k, **p)
        assert got['link_seg'][s].tolist() == [len(mine), paths, 0, 0], s
        assert got['link_rows'][s, :len(mine)].tolist() == want, (s, mine)
    return got


@pytest.mark.parametrize('n', [0, 1, 2, 63, 64])
def test_segment_sizes(world, n):
    assert_rows(world, [cases.staircase_case(n)], max_chains=64)      # lane 63 holds a chain at n = 64
    pick = [m for m in cases.fuzz_segments(90 + n, 50) if len(m) >= n][0][:n]
    assert len(pick) == n
    assert_rows(world, [pick], max_chains=max(n, 1), **cases.FUZZ_SMALL)
    assert_rows(world, [pick], max_chains=64, **cases.FUZZ_SMALL)


@pytest.mark.parametrize('nseg', [1, 2, 5])
def test_segment_routing_with_empty_segments_among_full_ones(world, nseg):
    full = [cases.staircase_case(64), cases.isolated_case(64), cases.shared_predecessor_case()]
    segments = {1: [full[0]], 2: [[], full[0]], 5: [[], full[1], [], full[2], full[0]]}[nseg]
    assert_rows(world, segments, max_chains=64)
    assert_rows(world, [[]] * nseg, max_chains=3)


def test_thresholds(world):
    for label, mine, p, want in cases.threshold_cases():
        got = assert_rows(world, [mine], **p)
        assert int(got['link_rows'][0, 1, 3]) == want, label


def test_ties_and_scores(world):
    mine, want = cases.order_case()
    assert assert_rows(world, [mine])['link_rows'][0, :, 0].tolist() == want
    for flip in (False, True):
        mine, winner = cases.equal_candidates_case(flip)
        assert int(assert_rows(world, [mine])['link_rows'][0, 2, 2]) == winner
    got = assert_rows(world, [cases.equal_f_case()])
    assert got['link_rows'][0, :, 4].tolist() == [1, 0]        # equal F: the smaller rank, chain 1, is path 0


def test_path_shapes(world):
    got = assert_rows(world, [cases.shared_predecessor_case(), cases.staircase_case(), cases.isolated_case()], max_chains=64)
    assert got['link_rows'][0, :3, 4].tolist() == [0, 0, 1] and got['link_rows'][0, :3, 6].tolist() == [190, 0, 34]
    assert got['link_seg'][:, 1].tolist() == [2, 1, 64]
    assert got['link_rows'][1, :, 5].tolist() == list(range(64)) and sorted(got['link_rows'][2, :, 4].tolist()) == list(range(64))


def test_fuzz_of_300_segments(world):
    assert_rows(world, cases.fuzz_segments(5, 300), max_chains=64, **cases.FUZZ_SMALL)       # small ranges: ties abound
    assert_rows(world, cases.fuzz_segments(5, 75, wide=True), max_chains=64)                  # beside them: introns and back-splices at the defaults


def test_refusals(world):
    counts, rows = planted([cases.shared_predecessor_case()])
    for p in (dict(max_query_gap=-1), dict(max_overlap=-1), dict(max_skew=-1), dict(max_intron=-1), dict(max_circle=-1), dict(intron_cost=-1),
              dict(backsplice_cost=-1), dict(max_skew=501, max_intron=500), dict(intron_cost=1 << 40), dict(backsplice_cost=1 << 40)):
        with pytest.raises(hip.ClhError, match=r'clh_seed_link_rows failed \(-2\)'):
            world.link_rows(counts, rows, **p)
        with pytest.raises(hip.ClhError, match=r'clh_seed_link_batch failed \(-2\)'):
            world.links(['ACGT' * 20], **p)
    for max_chains in (0, 65):
        with pytest.raises(hip.ClhError, match=r'clh_seed_link_batch failed \(-2\).*max_chains'):
            world.links(['ACGT' * 20], max_chains=max_chains)
    with pytest.raises(hip.ClhError, match=r'clh_seed_link_rows failed \(-2\).*max_chains'):
        world.link_rows(np.zeros(1, dtype=np.int64), np.zeros((1, 65, 10), dtype=np.int64))
    for count in (-1, 4):
        with pytest.raises(hip.ClhError, match=r'\(-2\).*segment 1 has %d chains' % count):
            world.link_rows(np.array([3, count]), np.concatenate([rows, rows]))
    for field, value in ((5, -1), (6, 1 << 40), (7, 1 << 40), (8, -1), (3, 1 << 40), (3, -(1 << 40))):
        bad = np.concatenate([rows, rows])
        bad[1, 2, field] = value
        with pytest.raises(hip.ClhError, match=r'\(-2\).*segment 1, chain 2'):
            world.link_rows(np.array([3, 3]), bad)
        bad[1, 2, field] = (1 << 40) - 1 if value > 0 else 0 if field != 3 else 1 - (1 << 40)      # on the bound: taken, and answered as the checker does
        got = world.link_rows(np.array([3, 3]), bad)
        for s in (0, 1):
            mine = [cases.chain(*(int(bad[s, c, f]) for f in (2, 3, 5, 7, 6, 8))) for c in range(3)]
            want, paths = lc.rows(mine, world.k)
            assert got['link_seg'][s].tolist() == [3, paths, 0, 0] and got['link_rows'][s].tolist() == want, (field, value, s)
    assert_rows(world, [cases.shared_predecessor_case()], max_skew=0, max_intron=0, max_circle=0, max_query_gap=0, max_overlap=0, intron_cost=0,
                backsplice_cost=0)


def raw_segments(got, r):
    """the chains of read r out of the raw arrays of SeedIndex.links: [plus, minus], as the checker holds them"""
    names = ('read', 'minus', 'contig', 'score', 'anchors', 'x_first', 'y_first', 'x_end', 'y_end')
    out = []
    for s in (2 * r, 2 * r + 1):
        mine = [dict(zip(names, got['rows'][s, c, :9].tolist())) for c in range(int(got['seg'][s, 0]))]
        for c in mine:
            assert c.pop('read') == r
        out.append(mine)
    return out


def test_links_of_planted_reads_equal_the_checker_in_one_share_and_in_two(world):
    genome, want_idx, _ = cases.checked()
    texts = [r['text'] for r in cases.reads()]
    got = world.links(texts)
    assert world.info()['shares'] == 1
    for r, text in enumerate(texts):
        segs = lc.segment_chains(genome, want_idx, sc.encode(text), cases.K, cases.W, cases.MAX_OCC)
        assert raw_segments(got, r) == segs, r                # the chain rows, in the order the chain kernel emits them
        for minus in (0, 1):
            want, paths = lc.rows(segs[minus], cases.K)
            s = 2 * r + minus
            assert got['link_seg'][s].tolist() == [len(segs[minus]), paths, 0, 0] and got['link_rows'][s, :len(segs[minus])].tolist() == want, (r, minus)
    anchors = world.seeds(texts)['anchor_off']
    cut = world.links(texts, workspace_bytes=64 * int(anchors[-1]) // 2 + 64 * int(np.diff(anchors).max()))
    assert world.info()['shares'] >= 2
    for name in got:                                         # the rows behind a segment's count keep the marker in both
        assert (got[name] == cut[name]).all(), name
    assert world.timing()['link'] > 0


def test_link_reads_and_link_chains_equal_the_checker(world):
    genome, want_idx, want = cases.checked()
    reads = cases.reads()
    texts = [r['text'] for r in reads]
    got = seed.link_reads(world, texts)
    assert got == want
    for r, read in enumerate(reads):                         # the truth the checker was asserted to carry, through the device
        if not read['errors']:
            assert got[r][0]['links'].count('backsplice') == (1 if read['what'] == 'circle' else 0), r
            assert ('circle' in got[r][0]) == (read['what'] == 'circle'), r
    for params in (dict(min_path_score=150), dict(max_chains=3), dict(max_intron=1500, backsplice_cost=90, intron_cost=0), dict(max_skew=700, max_circle=1200)):
        got = seed.link_reads(world, texts, **params)
        assert got == [lc.link_read(genome, want_idx, sc.encode(t), cases.K, cases.W, cases.MAX_OCC, **dict(params)) for t in texts], params
    lists = [[c for path in mine for c in path['chains']] for mine in want]
    lengths = [len(t) for t in texts]
    assert seed.link_chains(world, lists, lengths) == lc.link_chains(genome.names, lists, lengths, cases.K)
    assert seed.link_chains(world, [[], lists[0]], [10, lengths[0]], backsplice_cost=500) == lc.link_chains(genome.names, [[], lists[0]], [10, lengths[0]], cases.K,
                                                                                                          backsplice_cost=500)


def test_map_spliced_gives_the_planted_exons(world):
    genome, want_idx, want = cases.checked()
    reads = cases.reads()
    texts = [r['text'] for r in reads]
    got = seed.map_spliced(world, texts)
    windows, queries = [], []
    for r, read in enumerate(reads):
        path = got[r]
        assert {k: v for k, v in path.items() if k != 'pieces'} == {k: v for k, v in want[r][0].items() if k != 'pieces'}, r
        assert [{k: p[k] for k in ('ref_start', 'ref_end', 'query_start', 'query_end')} for p in path['pieces']] == want[r][0]['pieces'], r
        for window, query in lc.spliced_pieces(want[r][0], sc.encode(read['text'])):
            windows.append(window)
            queries.append(np.array(query, dtype=np.int8))
    direct = ssw_wrap.align_windows_spliced(world.genome, windows, queries, mode='global', strand='both', report_cigar=True)
    flat = [p for path in got for p in path['pieces']]
    assert len(flat) == len(direct)
    for piece, res in zip(flat, direct):
        assert (piece['exons'], piece['strand'], piece['score'], piece['cigar_string']) == (res.exons, res.strand, res.score, res.cigar_string)
    _, genes = cases.world()
    for r, read in enumerate(reads):
        if read['errors']:
            continue
        for piece, exons in zip(got[r]['pieces'], cases.expected_pieces(read)):
            assert len(piece['exons']) == len(exons), (r, piece, exons)
            # the interior boundaries are the planted ones; the outer ends are the anchors'
            assert [a for a, _ in piece['exons'][1:]] == [a for a, _ in exons[1:]] and [b for _, b in piece['exons'][:-1]] == [b for _, b in exons[:-1]], r
            if len(exons) > 1:
                assert piece['strand'] == genes[read['gene']][1], r
            assert piece['cigar_string'].count('N') == len(exons) - 1 and not set(piece['cigar_string']) & set('IDS'), r
