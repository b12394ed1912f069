"""The link kernel, K7j and K7c on the GPU (csrc/seed_link.hip, seed_junction.hip, seed_circle.hip) at the edges their feature tests leave
out, every array compared for equality with the plain statements (tests/link_check.py, junction_check.py, circle_check.py).  The inputs
are those of tests/k7_edges.py, which tests/test_k7_edges_host.py proves to be what they claim with the checkers alone: negative F and
the 2^40 bound in the link step; ties, clipped windows and the scoring bound 2^20 - 1 in K7j's classes of 2, 4 and 8 rows per lane; in
K7c a read that fills every task slot, other strides, batches across the 256-thread workgroups with one circle of more than 256 reads,
starts above 2^16 in a contig-major table, and the full read as a share of its own."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import circle_cases as ccases  # noqa: E402
import k7_edges as edges  # noqa: E402
import link_cases as lcases  # noqa: E402
from ciri_long_amd import hip, seed  # noqa: E402
from test_gpu_circles import assert_equal  # noqa: E402
from test_gpu_junction import assert_batch  # noqa: E402
from test_gpu_link import assert_rows  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


def indexed(ctx, contigs):
    genome = hip.Genome(ctx, contigs)
    idx = seed.index(genome, k=edges.K, w=edges.W, max_occ=edges.MAX_OCC)
    yield idx
    idx.close()
    genome.close()


@pytest.fixture(scope='module')
def link_world(ctx):
    """link_rows reads no genome: link_cases' world stands in"""
    yield from indexed(ctx, lcases.world()[0])


@pytest.fixture(scope='module')
def planted_world(ctx):
    """circle_cases' world"""
    yield from indexed(ctx, ccases.world()[0])


@pytest.fixture(scope='module')
def full_world(ctx):
    """circle_cases' world and the contig of the full read behind it"""
    yield from indexed(ctx, edges.full_world()[0])


@pytest.fixture(scope='module')
def far_world(ctx):
    yield from indexed(ctx, edges.far_world()[0])


# ---- link kernel ---------------------------------------------------------------------------------------------------------------------

def test_link_negative_f(link_world):
    for label, mine, p in edges.negative_cases():
        got = assert_rows(link_world, [mine], **p)
        assert_rows(link_world, [mine], max_chains=64, **p)
        if label.startswith('all negative'):
            assert (got['link_rows'][0, :, 1] < 0).all() and (got['link_rows'][0, :, 6] < 0).all() and int(got['link_seg'][0, 1]) == len(mine)
    assert_rows(link_world, [mine for _, mine, _ in edges.negative_cases()], max_chains=64)      # side by side, the waves of three workgroups


def test_link_top_of_the_range(link_world):
    T = edges.TOP
    for label, mine, p in edges.top_cases():
        got = assert_rows(link_world, [mine], **p)
        if label == 'staircase of 64':
            assert int(got['link_rows'][0, 63, 1]) == 64 * T - 63 * 16 and got['link_rows'][0, :, 5].tolist() == list(range(64))
        if label == 'costs':
            assert got['link_rows'][0, :, 1].tolist() == [T, 2 * T, T + 5, T + 7] and got['link_rows'][0, :, 3].tolist() == [0, 1, 2, 3]


def test_link_fuzz_over_negative_zero_small_and_near_bound_scores(link_world):
    for segments, p in edges.range_fuzz():
        assert_rows(link_world, segments, max_chains=64, **p)


@pytest.mark.parametrize('nseg', [3, 4, 8, 9])
def test_link_segment_counts_around_a_workgroup(link_world, nseg):
    got = assert_rows(link_world, edges.workgroup_segments(nseg), max_chains=64)
    assert int(got['link_seg'][nseg - 1, 0]) == 64


# ---- K7j -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('cls', [1, 2, 3])
def test_junction_ties_in_the_classes_of_several_rows_per_lane(ctx, cls):
    (planted, batch), = [(p, b) for c, p, b in edges.slide_batches() if c == cls]
    got = assert_batch(ctx, batch)
    for n, (slide, a, want) in enumerate(planted):
        assert got[n, 2:4].tolist() == [1 if want < 0 else 0, a], (slide, a, want)      # strand + where it may be, the first t of the tie


def test_junction_low_complexity_fuzz_in_classes_1_2_3(ctx):
    for batch in edges.class_fuzz_batches():
        assert_batch(ctx, batch)


def test_junction_windows_clipped_inside_classes_1_2_3(ctx):
    batch = edges.clip_batch()
    got = assert_batch(ctx, batch)
    assert got[0, 4:8].tolist() == [0, 0, len(batch[0][1][1]), 0] and got[0, 10:12].tolist() == [6, 6]


@pytest.mark.parametrize('name', ['planted', 'unrelated', 'poly'])
def test_junction_scoring_on_the_bound_at_the_full_span(ctx, name):
    got = assert_batch(ctx, edges.bound_batches()[name])
    if name == 'poly':
        assert (got[:, 1] < 0).all() and int(got[:, 8:10].min()) < -400000


# ---- K7c -----------------------------------------------------------------------------------------------------------------------------

def test_circle_read_that_fills_every_slot(full_world):
    texts = edges.full_texts()
    for r in (edges.FULL_READ, edges.FULL_READ + 1):     # alone, and as its reverse complement
        got = full_world.circles([texts[r]], **edges.FULL)
        assert_equal(got, edges.expected([texts[r]], 64))
        assert got['circle'][0, 11:14].tolist() == [64, 63, 62]
    batch = edges.middle_batch()
    assert_equal(full_world.circles(batch, **edges.FULL), edges.expected(batch, 64))


@pytest.mark.parametrize('max_chains', [16, 2, 1])
def test_circle_full_read_at_fewer_slots(full_world, max_chains):
    texts = edges.full_texts()
    batch = [texts[edges.FULL_READ], texts[0], texts[edges.FULL_READ + 1]]
    assert_equal(full_world.circles(batch, **dict(edges.FULL, max_chains=max_chains)), edges.expected(batch, max_chains))


@pytest.mark.parametrize('max_chains', [1, 2, 3, 64])
def test_circle_planted_reads_at_other_strides(planted_world, max_chains):
    assert_equal(planted_world.circles(ccases.texts(), **ccases.link_of(max_chains)), ccases.want(max_chains=max_chains))


@pytest.mark.parametrize('n,hub,last', edges.BATCHES, ids=['255', '256-circle-last', '256-none-last', '257', '513-hub'])
def test_circle_batches_across_the_workgroups(full_world, n, hub, last):
    texts = edges.full_texts()
    order = edges.cycled(n, hub, last)
    want = edges.expected([texts[r] for r in order])
    got = full_world.circles([texts[r] for r in order], **ccases.LINK)
    assert_equal(got, want, order)
    if hub:                                             # more than 256 reads of one circle, from every workgroup of the batch
        g = int(got['circle_of_read'][0])
        members = np.flatnonzero(got['circle_of_read'] == g)
        assert len(members) > 256 and got['table'][g, 6:9].tolist() == [len(members), int(got['circle'][members, 7].max()), 0]


def test_circle_starts_above_65536_in_a_contig_major_table(far_world):
    _, circles, reads = edges.far_world()
    got = far_world.circles([t for _, t in reads], **ccases.LINK)
    assert_equal(got, edges.far_want()[1])
    assert [tuple(t[:3]) for t in got['table'].tolist()] == [circles[name] for name in ('short', 'long', 'near', 'low')]


def test_circle_full_read_as_a_share_of_its_own(full_world):
    texts = edges.full_texts()
    order = edges.share_batch()
    batch = [texts[r] for r in order]
    one = full_world.circles(batch, **ccases.LINK)
    assert full_world.info()['shares'] == 1
    anchors = full_world.seeds(batch)['anchor_off'].tolist()
    at = order.index(edges.FULL_READ)
    cap = anchors[at + 1] - anchors[at]                 # the full read's own anchors: it fits a share, and nothing with anchors fits beside it
    shares = edges.greedy_shares(anchors, cap)
    mine = shares.index((at, at + 1))
    assert 0 < mine < len(shares) - 1 and shares[mine - 1][1] - shares[mine - 1][0] > 1 and shares[mine + 1][1] - shares[mine + 1][0] > 1
    cut = full_world.circles(batch, workspace_bytes=64 * cap, **ccases.LINK)
    assert full_world.info()['shares'] == len(shares) >= 3
    for name in ('circle', 'circle_of_read', 'table'):
        assert (one[name] == cut[name]).all(), name
    assert_equal(cut, edges.expected(batch))
