"""K7c on the GPU (csrc/seed_circle.hip): the circles of a read batch in one device pass, every array compared for equality with the
plain statement tests/circle_check.py and, through seed.circle_dicts, with the composed route seed.call_circles that existed before it.
The planted reads are those of tests/circle_cases.py, which tests/test_circle_host.py asserts with the checkers alone: all four
statuses, strands that tie, two turns of a circle, junctions too wide to refine, circles at a contig's end, N and lower-case flanks,
one circle read on both strands, widths across K7j's class bound; and shares, routing, refusals and the unchanged neighbours."""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import circle_cases as cases  # noqa: E402
import circle_check as cc  # noqa: E402
from ciri_long_amd import hip, seed  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def world(ctx):
    """the planted genome on the device with its index at k = 15, w = 5"""
    genome = hip.Genome(ctx, cases.world()[0])
    idx = seed.index(genome, k=cases.K, w=cases.W, max_occ=cases.MAX_OCC)
    yield idx
    idx.close()
    genome.close()


def assert_equal(got, want, order=None):
    """got: what SeedIndex.circles gave; want: (rows, circle_of_read, table) of the checker, for the reads in `order`"""
    rows, where, tab = want
    assert got['circle'].dtype == got['circle_of_read'].dtype == got['table'].dtype == np.int64
    assert got['circle'].shape == (len(rows), cc.ROW) and got['table'].shape == (len(tab), cc.TABLE)
    for r, (g, w) in enumerate(zip(got['circle'].tolist(), rows)):
        assert g == w, (r, order[r] if order else r)
    assert got['circle_of_read'].tolist() == where
    assert got['table'].tolist() == tab
    assert got['kernel_ms'].shape == (3,) and (got['kernel_ms'] >= 0).all()


def test_arrays_equal_the_checker_on_all_planted_reads(world):
    got = world.circles(cases.texts(), **cases.LINK)
    assert_equal(got, cases.want())
    assert set(got['circle'][:, 0].tolist()) == {0, 1, 2, 3} and got['kernel_ms'][1] > 0
    assert_equal(world.circles(cases.texts(), **dict(cases.LINK, **cases.SCORING)), cases.want(True))
    assert_equal(world.circles(cases.texts(), min_path_score=200, **cases.LINK), cases.want(False, 200))


@pytest.mark.parametrize('more', [{}, cases.SCORING, dict(min_path_score=200)], ids=['default', 'scoring', 'min_path_score'])
def test_circle_dicts_equal_call_circles_but_for_the_path(world, more):
    texts = cases.texts()
    old = seed.call_circles(world, texts, **dict(cases.LINK, **more))
    new = seed.call_circles_batch(world, texts, **dict(cases.LINK, **more))
    mine = seed.circle_dicts(world, new)
    assert len(old) == len(mine) == len(texts)
    for r, (a, b) in enumerate(zip(old, mine)):
        assert ({k: v for k, v in a.items() if k != 'path'} if a else None) == b, (r, cases.reads()[r][0])
    assert sum(1 for b in mine if b) >= 20 and sum(1 for b in mine if not b) >= 10
    genome = cases.checked()[0]
    assert new['circles'] == cc.table_dicts(genome, new['table'].tolist())
    assert {'-AG', 'GT-', 'GN-AG'} <= {t['signal'] for t in new['circles']} or more
    assert sum(t['reads'] for t in new['circles']) == sum(1 for b in mine if b)


def test_three_shares_give_what_one_share_gives(world):
    texts = cases.texts()
    one = world.circles(texts, **cases.LINK)
    assert world.info()['shares'] == 1
    anchors = world.seeds(texts)['anchor_off']
    most = int(np.diff(anchors).max())
    cut = world.circles(texts, workspace_bytes=64 * max(most, int(anchors[-1]) // 4), **cases.LINK)
    assert world.info()['shares'] >= 3
    for name in ('circle', 'circle_of_read', 'table'):
        assert (one[name] == cut[name]).all(), name
    assert_equal(cut, cases.want())
    with pytest.raises(hip.ClhError, match=r'clh_seed_circle_batch failed \(-4\).*anchors'):
        world.circles(texts, workspace_bytes=64 * (most - 1), **cases.LINK)


def test_routing_over_more_reads_than_a_workgroup_holds_with_the_statuses_interleaved(world):
    texts = cases.texts()
    rows = cases.want()[0]
    by = {s: [r for r, v in enumerate(rows) if v[0] == s] for s in range(4)}
    found = by[0] * 2
    random.Random(8).shuffle(found)
    order = []
    for at, r in enumerate(found):                      # behind every read with a circle one without, of status 1, 2, 3 in turn
        other = by[1 + at % 3]
        order += [r, other[(at // 3) % len(other)]]
    statuses = [rows[r][0] for r in order]
    assert len(order) > 64 and all(set(statuses[a:a + 8]) == {0, 1, 2, 3} for a in range(len(order) - 8))
    want_rows = [rows[r] for r in order]                # the read's index is the only word of a task that the order changes; no row holds it
    tab, where = cc.table(want_rows)
    got = world.circles([texts[r] for r in order], **cases.LINK)
    assert_equal(got, (want_rows, where, tab), order)
    assert [t[6] for t in got['table'].tolist()] == [2 * t[6] for t in cases.want()[2]]


def test_no_read_one_read_and_an_empty_read(world):
    got = world.circles([], **cases.LINK)
    assert got['circle'].shape == (0, 16) and got['circle_of_read'].shape == (0,) and got['table'].shape == (0, 10)
    rows = cases.want()[0]
    for name in ('empty', 'junction_cases 0', 'linear', 'too wide'):
        r = cases.label(name)
        got = world.circles([cases.texts()[r]], **cases.LINK)
        tab, where = cc.table([rows[r]])
        assert_equal(got, ([rows[r]], where, tab))
    got = world.circles(['', ''], **cases.LINK)
    assert got['circle'].tolist() == [[1] + [0] * 15] * 2 and got['circle_of_read'].tolist() == [-1, -1] and len(got['table']) == 0


def test_junction_classes_on_either_side_of_64(world):
    """widths of 63, 64 and 65 letters between the anchors (tests/test_circle_host.py proves them planted): K7j's first and second class"""
    _, link_p, _ = cc.split(cases.LINK)
    picked = {}
    for r, segs in enumerate(cases.segments()):
        best = cc.best_path(segs, cases.K, 0, **link_p)
        for t in (cc.tasks(r, best[0], segs[best[0]], best[2], best[3], cases.K) if best else []):
            if t[6] - t[4] in (63, 64, 65):
                picked.setdefault(t[6] - t[4], r)
    assert sorted(picked) == [63, 64, 65]
    rows = cases.want()[0]
    order = [picked[m] for m in (65, 63, 64)]
    tab, where = cc.table([rows[r] for r in order])
    assert_equal(world.circles([cases.texts()[r] for r in order], **cases.LINK), ([rows[r] for r in order], where, tab))


def test_reverse_complements_name_the_same_circles(world):
    texts = cases.texts()
    fwd = world.circles(texts, **cases.LINK)
    rev = world.circles([cases.rc(t) for t in texts], **cases.LINK)
    palindromes = {cases.label('palindrome a'), cases.label('palindrome b')}
    for r, (a, b) in enumerate(zip(fwd['circle'].tolist(), rev['circle'].tolist())):
        assert a[:8] == b[:8] and a[10:] == b[10:], (r, a, b)
        if a[0] != cc.NO_PATH:
            assert a[9] == (b[9] if r in palindromes else 1 - b[9]), r
        if a[0] == cc.FOUND:
            assert a[8] == (b[8] if r in palindromes else len(texts[r]) - b[8]), r
    assert (fwd['table'][:, :8] == rev['table'][:, :8]).all() and (fwd['circle_of_read'] == rev['circle_of_read']).all()


def test_refusals(world):
    texts = ['ACGT' * 20, 'ACGTNACGT']
    assert world.circles(texts)['circle'][:, 0].tolist() == [1, 1]
    name = r'clh_seed_circle_batch failed \(-2\).*clh_seed_circle_batch: '
    for p in (dict(max_query_gap=-1), dict(max_overlap=-1), dict(max_skew=-1), dict(max_intron=-1), dict(max_circle=-1), dict(intron_cost=-1),
              dict(backsplice_cost=-1), dict(max_skew=501, max_intron=500), dict(intron_cost=1 << 40), dict(backsplice_cost=1 << 40),
              dict(max_chains=0), dict(max_chains=65), dict(lookback=0), dict(lookback=65), dict(max_attempts=0), dict(max_gap=-1),
              dict(max_span=0), dict(max_span=513), dict(slack=-1), dict(slack=65), dict(match=-1), dict(mismatch=-1), dict(gap_open=-1, gap_extend=-1),
              dict(gap_extend=-1), dict(match=1 << 20), dict(max_span=100, slack=16, match=4800, intron_open=10000, noncanonical=888)):
        with pytest.raises(hip.ClhError, match=name):
            world.circles(texts, **p)
    with pytest.raises(hip.ClhError, match=r'clh_seed_circle_batch failed \(-3\).*clh_seed_circle_batch: '):
        world.circles(texts, gap_open=1, gap_extend=2)
    for p in (dict(intron_open=-1), dict(noncanonical=-1), dict(donor_costs={'GT': -1}), dict(acceptor_costs={'AG': -1})):      # refused before the library is asked
        with pytest.raises(ValueError):
            world.circles(texts, **p)
    assert world.circles(texts, min_path_score=-5)['circle'][:, 0].tolist() == [1, 1]       # a negative min_path_score is admitted
    data, off = hip.pack(texts)
    sp = hip.splice_of('test', 12, 6)
    sp.donor[3] = -1                                     # the library's own refusal of a negative cost
    o, lo, jo = hip.ChainOpts(64, 32, 256, 40, 3, 0, 5000, 500, 0), hip.LinkOpts(500, 32, 500, 200000, 200000, 16, 32), hip.JunctionOpts(2, 2, 3, 1, 16, 512)
    circle, where, count = np.zeros((2, 16), dtype=np.int64), np.zeros(2, dtype=np.int64), C.c_int64(7)
    call = hip.lib().clh_seed_circle_batch
    assert call(world._h, 2, data.ctypes.data, off.ctypes.data, C.byref(o), C.byref(lo), C.byref(jo), C.byref(sp), 0, circle.ctypes.data, where.ctypes.data, C.byref(count), None) == -2
    sp = hip.splice_of('test', 12, 6)
    for hole in range(8):                               # every pointer but kernel_ms
        args = [world._h, 2, data.ctypes.data, off.ctypes.data, C.byref(o), C.byref(lo), C.byref(jo), C.byref(sp), 0, circle.ctypes.data, where.ctypes.data, C.byref(count), None]
        args[(0, 3, 4, 5, 6, 7, 9, 10)[hole]] = None
        assert call(*args) == -2 and 'clh_seed_circle_batch: null argument' in hip.last_error()
    bad = off.copy()
    bad[1] = off[2] + 1
    with pytest.raises(hip.ClhError, match=name + 'offsets must ascend'):
        world.circles((data, bad))
    data[off[1] + 4] = 5
    with pytest.raises(hip.ClhError, match=name + r'read 1 holds a code outside 0\.\.4'):
        world.circles((data, off))
    got = world.circles(cases.texts()[:12], **cases.LINK)
    assert len(got['table']) >= 2
    small = np.zeros((len(got['table']) - 1, 10), dtype=np.int64)
    assert hip.lib().clh_seed_circle_table_fetch(world._h, len(small), small.ctypes.data) == -4 and 'cap too small' in hip.last_error()
    full = np.zeros((len(got['table']), 10), dtype=np.int64)
    assert hip.lib().clh_seed_circle_table_fetch(world._h, len(full), full.ctypes.data) == 0 and (full == got['table']).all()


def test_neighbours_are_unchanged_by_a_circles_call(world):
    texts = cases.texts()[:30]
    links = world.links(texts, **cases.LINK)
    paths = seed.link_reads(world, texts, **cases.LINK)
    tasks = np.array([[0, 0, 0, 300, 2, 100, 12, 0]], dtype=np.int64)
    rows = world.junctions(['ACGTACGTACGTACGTACGT'], tasks)
    world.circles(texts, **cases.LINK)
    assert sorted(world.timing()) == ['chain', 'link', 'seeds', 'sketch', 'sort'] and world.timing()['link'] > 0
    again = world.links(texts, **cases.LINK)
    for name in ('seg', 'rows', 'link_seg', 'link_rows'):
        assert (links[name] == again[name]).all(), name
    assert seed.link_reads(world, texts, **cases.LINK) == paths
    assert (world.junctions(['ACGTACGTACGTACGTACGT'], tasks) == rows).all()
