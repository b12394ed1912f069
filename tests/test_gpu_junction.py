"""K7j on the GPU (csrc/seed_junction.hip): back-splice junctions refined to the base, every row compared for equality with the plain
statement tests/junction_check.py.  The planted tasks and the planted circles are those of tests/junction_cases.py, which
tests/test_junction_host.py asserts with the checker alone: sizes around every class bound at slack 0, 16 and 64, routing over more tasks
than a workgroup holds, windows clipped at both contig ends, neighbouring contigs, code 4, soft-masked letters, minus reads, the tie
cases and the fuzz, the scoring edges, every refusal, and refine_junctions / call_circles / map_spliced(refine=True) end to end."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import junction_cases as cases  # noqa: E402
import junction_check as jc  # noqa: E402
import seed_check as sc  # noqa: E402
from ciri_long_amd import hip, seed  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def info():
    got = hip.SeedIndex.junction_info()
    assert got['class_bounds'] == sorted(got['class_bounds']) and got['class_bounds'][-1] == got['max_span'] == jc.MAX_SPAN and got['max_slack'] == jc.MAX_SLACK
    return got


@pytest.fixture(scope='module')
def world(ctx):
    """the planted genome on the device with its index at k = 15, w = 5"""
    contigs, _ = cases.world()
    genome = hip.Genome(ctx, contigs)
    idx = seed.index(genome, k=cases.K, w=cases.W, max_occ=cases.MAX_OCC)
    yield idx
    idx.close()
    genome.close()


def run(ctx, batch, **more):
    """a batch on the device -> its [n, 12] rows"""
    contigs, texts, tasks, scoring = batch
    genome = hip.Genome(ctx, contigs)
    idx = seed.index(genome, k=cases.K, w=cases.W, max_occ=cases.MAX_OCC)
    try:
        return idx.junctions(texts, np.array(tasks, dtype=np.int64).reshape(-1, 8), **dict(scoring, **more))
    finally:
        idx.close()
        genome.close()


def assert_batch(ctx, batch):
    got = run(ctx, batch)
    want = cases.want_rows(batch)
    assert got.shape == (len(want), 12)
    for n, (g, w) in enumerate(zip(got.tolist(), want)):
        assert g == w, (n, batch[2][n], batch[3])
    return got


@pytest.mark.parametrize('slack', [0, 16, 64])
def test_sizes_around_every_class_bound(ctx, info, slack):
    batch = [b for b in cases.size_batches(info['class_bounds'], info['max_span']) if b[3]['slack'] == slack][0]
    spans = sorted({t[6] - t[4] for t in batch[2]})
    assert spans == [0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513]
    got = assert_batch(ctx, batch)
    assert sorted(got[:, 0].tolist()).count(1) == 1 and sorted(got[:, 0].tolist()).count(2) == 2       # among valid ones


def test_no_task_and_one_task(ctx, info):
    batch = cases.routing_batch(info['class_bounds'], info['waves'])
    assert run(ctx, (batch[0], batch[1], [], batch[3])).shape == (0, 12)
    for n in (0, 17):
        assert_batch(ctx, (batch[0], batch[1], batch[2][n:n + 1], batch[3]))


def test_routing_of_interleaved_classes_and_many_tasks_on_one_read(ctx, info):
    batch = cases.routing_batch(info['class_bounds'], info['waves'])
    classes = [[b for b in range(len(info['class_bounds'])) if t[6] - t[4] <= info['class_bounds'][b]][0] for t in batch[2]]
    assert min(classes.count(b) for b in range(len(info['class_bounds']))) > 2 * info['waves'] and classes != sorted(classes)
    assert {t[7] for t in batch[2]} == {-1, 0, 1} and max(sum(1 for t in batch[2] if t[0] == r) for r in range(len(batch[1]))) == 40
    got = assert_batch(ctx, batch)
    assert set(got[:, 2].tolist()) == {0, 1}


def test_clipped_windows_neighbours_code_4_and_soft_masked_letters(ctx):
    batch = cases.window_batch()
    got = assert_batch(ctx, batch)
    first = batch[2][0]                                 # xd at the end of 'mid', in front of a contig that begins with GT; xa == 0 behind one that ends with AG
    assert (first[3], first[5]) == (120, 0) and got[0, 4:8].tolist() == [0, 0, 120, 0] and got[0, 10:12].tolist() == [6, 6]
    assert any('N' in t for t in batch[1]) and any(c != c.upper() for _, c in batch[0]) and any(t[1] for t in batch[2])


def test_ties(ctx):
    for slide, t0, batch in cases.slide_cases():
        got = assert_batch(ctx, batch)
        assert got[0, 2:4].tolist() == [0, t0]
    for batch in cases.fuzz_batches():
        assert_batch(ctx, batch)


def test_scoring_edges_and_costs_just_under_the_bound(ctx):
    for batch in cases.score_batches():
        assert_batch(ctx, batch)


def test_refusals(ctx, world):
    texts = ['ACGTACGTACGTACGTACGT', 'ACGTNACGT']
    size = world.genome.length['j0']
    ok = np.array([[0, 0, 0, 300, 2, 100, 12, 0]], dtype=np.int64)
    assert world.junctions(texts, ok)[0, 0] == 0
    for p in (dict(max_span=0), dict(max_span=513), dict(slack=-1), dict(slack=65), dict(match=-1), dict(mismatch=-1), dict(gap_open=-1, gap_extend=-1),
              dict(gap_extend=-1), dict(match=1 << 20), dict(max_span=100, slack=16, match=4800, intron_open=10000, noncanonical=888)):
        assert jc.admitted(jc.parameters(p)) == -2
        with pytest.raises(hip.ClhError, match=r'clh_seed_junction_batch failed \(-2\)'):
            world.junctions(texts, ok, **p)
    with pytest.raises(hip.ClhError, match=r'clh_seed_junction_batch failed \(-3\)'):
        world.junctions(texts, ok, gap_open=1, gap_extend=2)
    for p in (dict(intron_open=-1), dict(noncanonical=-1), dict(donor_costs={'GT': -1}), dict(acceptor_costs={'AG': -1})):      # refused before the library is asked
        with pytest.raises(ValueError):
            world.junctions(texts, ok, **p)
    sp = hip.splice_of('test', 12, 6)
    sp.donor[3] = -1                                     # the library's own refusal of a negative cost
    out = np.zeros((1, 12), dtype=np.int64)
    data, off = hip.pack(texts)
    o = hip.JunctionOpts(2, 2, 3, 1, 16, 512)
    import ctypes as C
    assert hip.lib().clh_seed_junction_batch(world._h, 2, data.ctypes.data, off.ctypes.data, 1, ok.ctypes.data, C.byref(o), C.byref(sp), out.ctypes.data, None) == -2
    for field, value, what in ((0, -1, 'read'), (0, 2, 'read'), (2, -1, 'contig'), (2, 4, 'contig'), (4, -1, 'yd'), (4, 21, 'yd'), (6, -1, 'ya'), (6, 21, 'ya'),
                               (3, -1, 'xd'), (3, size + 1, 'xd'), (5, -1, 'xa'), (5, size + 1, 'xa'), (7, 2, 'strand'), (7, -2, 'strand')):
        bad = np.concatenate([ok, ok, ok])
        bad[1, field] = value
        with pytest.raises(hip.ClhError, match=r'\(-2\).*task 1: .*%s' % what):
            world.junctions(texts, bad)
    edge = np.array([[0, 0, 0, size, 0, 0, 20, 0], [0, 1, 0, size, 20, size, 20, -1]], dtype=np.int64)      # on the bounds: taken
    assert world.junctions(texts, edge)[:, 0].tolist() == [0, 2]
    data[off[1] + 4] = 5
    with pytest.raises(hip.ClhError, match=r'\(-2\).*read 1 holds a code outside 0\.\.4'):
        world.junctions((data, off), ok)


def test_refine_junctions_and_call_circles_on_the_planted_reads(world):
    genome, _, paths = cases.checked()
    reads = cases.reads()
    texts = [r['text'] for r in reads]
    linked = seed.link_reads(world, texts, **cases.LINK)
    assert linked == paths
    got = seed.refine_junctions(world, texts, linked)
    assert got == cases.refined()
    for params in (dict(slack=0, max_span=40), dict(match=1, mismatch=3, gap_open=4, gap_extend=2, intron_open=0, noncanonical=2, donor_costs={'GC': 1})):
        assert seed.refine_junctions(world, texts, linked, **params) == [jc.refine_paths(genome, sc.encode(t), mine, cases.K, **params) for t, mine in zip(texts, paths)]
    circles = seed.call_circles(world, texts, **cases.LINK)
    assert circles == [jc.circle_of(mine[0]) if mine else None for mine in cases.refined()]
    for read, circle in zip(reads, circles):
        if not read['errors']:                          # the planted truth, to the base
            assert (circle['contig'], circle['start'], circle['end'], circle['strand'], circle['signal']) == (read['contig'],) + read['circle'] + (read['strand'], 'GT-AG')
            assert circle['circ_id'] == '%s:%d-%d' % (read['contig'], read['circle'][0] + 1, read['circle'][1])


def test_genome_letters_of_many_short_spans(ctx):
    contigs = cases.window_batch()[0]                    # N, lower-case letters, four contigs side by side
    genome = hip.Genome(ctx, contigs)
    try:
        windows = [(name, a, min(a + n, len(text))) for name, text in contigs for n in (0, 1, 2, 7) for a in range(0, len(text) + 1, 3)]
        assert len(windows) > 300
        text_of = dict(contigs)
        assert genome.letters(windows) == [''.join(c if c in 'ACGT' else 'N' for c in text_of[name][a:b].upper()) for name, a, b in windows]
        assert genome.letters([]) == [] and genome.letters([('mid', 5, 5)]) == ['']
        with pytest.raises(hip.ClhError, match=r'clh_genome_letters failed \(-2\)'):
            genome.letters([('soft', 160, 165)])        # the last contig: beyond the genome
    finally:
        genome.close()


def test_map_spliced_takes_the_junction_keywords_with_refine_alone(world):
    texts = [r['text'] for r in cases.reads()][:2]
    for name in ('slack', 'max_span'):
        with pytest.raises(TypeError):
            seed.map_spliced(world, texts, **dict(cases.LINK, **{name: 8}))
    got = seed.map_spliced(world, texts, refine=True, slack=8, max_span=64, **cases.LINK)
    assert [p['junctions'] for p in got] == [jc.refine_paths(cases.checked()[0], sc.encode(t), mine[:1], cases.K, slack=8, max_span=64)[0]['junctions']
                                             for t, mine in zip(texts, cases.checked()[2])]


def test_map_spliced_refined_tiles_the_planted_circle(world):
    reads = cases.reads()
    texts = [r['text'] for r in reads]
    plain = seed.map_spliced(world, texts, **cases.LINK)
    got = seed.map_spliced(world, texts, refine=True, **cases.LINK)
    again = seed.map_spliced(world, texts, refine=False, **cases.LINK)
    assert again == plain and all('junctions' not in p for p in plain if p)
    want = cases.refined()
    for r, read in enumerate(reads):
        if got[r] is None:
            assert not want[r]
            continue
        assert got[r]['junctions'] == want[r][0]['junctions'], r
        keys = ('ref_start', 'ref_end', 'query_start', 'query_end')
        assert [{k: p[k] for k in keys} for p in got[r]['pieces']] == jc.refined_pieces(want[r][0]), r
        if read['errors']:
            continue
        exons = [e for p in got[r]['pieces'] for e in p['exons']]
        planted = cases.expected_exons(read)
        assert (got[r]['pieces'][1]['exons'][0][0], got[r]['pieces'][0]['exons'][-1][1]) == (read['circle'][0], read['circle'][1] - 1), r
        for piece, mine in zip(got[r]['pieces'], planted):
            assert len(piece['exons']) == len(mine), (r, piece, mine)
            assert [a for a, _ in piece['exons'][1:]] == [a for a, _ in mine[1:]] and [b for _, b in piece['exons'][:-1]] == [b for _, b in mine[:-1]], r
            assert not set(piece['cigar_string']) & set('IDS'), r
        assert exons and plain[r]['pieces'] != got[r]['pieces']
