"""The edge cases of tests/k7_edges.py on the CPU: that each is what it claims to be, proved with the checkers alone (link_check,
junction_check, circle_check) before tests/test_gpu_k7_edges.py asks the GPU about the same inputs -- negative F and the 2^40 bound in
the link step, planted ties and clipped windows in K7j's classes of 2, 4 and 8 rows per lane, the scoring bound 2^20 - 1 at the full
span, a read that fills every task slot of K7c, batches across 256 reads with a circle of more than 256 of them, and a contig-major
table with starts above 2^16.  No GPU is touched."""
import collections
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import circle_cases as ccases  # noqa: E402
import circle_check as cc  # noqa: E402
import junction_cases as jcases  # noqa: E402
import junction_check as jc  # noqa: E402
import k7_edges as edges  # noqa: E402
import link_cases as lcases  # noqa: E402
import link_check as lc  # noqa: E402


def cls_of(m):
    return [b for b in range(4) if m <= 64 << b][0]


# ---- link kernel ---------------------------------------------------------------------------------------------------------------------

def test_link_negative_cases_hold_negative_f_in_every_role():
    by = {label: lc.link(mine, 15, **p) for label, mine, p in edges.negative_cases()}
    assert {len(mine) for label, mine, _ in edges.negative_cases() if 'alternating' in label} == {2, 63, 64}
    for n in (2, 63, 64):
        F, pred, kind, paths = by['all negative %d' % n]
        assert max(F) < 0 and set(pred) == {-1} and len(paths) == n and all(score < 0 for score, _ in paths)
        assert [score for score, _ in paths] == sorted(F, reverse=True) and (n == 2 or len(set(F)) < n)      # extraction among equal negative F
        F, pred, kind, paths = by['alternating %d' % n]
        linked = [c for c in range(n) if pred[c] >= 0]
        assert linked and any(F[c] <= 0 for c in linked) and any(score < 0 for score, _ in paths)   # a winner whose own F is not above 0
        if n > 2:
            assert any(F[c] > 0 for c in linked) and min(F) < 0 < max(F) and len(paths) > 1
    F, pred, kind, paths = by['negative path']
    assert pred == [-1, 0, 0] and F == [100, 190, 34] and paths == [(190, [0, 1]), (-66, [2])]      # the walk stops on chain 0: 34 - 100
    assert by['value 1, F below 0'][0] == [17, -79] and by['value 1, F below 0'][2] == [0, 2]
    assert by['value 1, F 0'][0] == [17, 0] and by['value 1, F 0'][1] == [-1, 0]
    assert by['value 0, F below 0'][0] == [16, -80] and by['value 0, F below 0'][1] == [-1, -1]


def test_link_top_cases_reach_the_bound_and_stay_exact():
    T = edges.TOP
    assert T == (1 << 40) - 1
    by = {label: (mine, lc.link(mine, 15, **p)) for label, mine, p in edges.top_cases()}
    mine, (F, pred, kind, paths) = by['coordinates and scores']
    assert {mine[1][f] for f in ('x_end', 'y_end')} == {T} and [c['score'] for c in mine] == [T, -T] and (F, pred, kind) == ([T, -16], [-1, 0], [0, 2])
    _, (F, pred, kind, paths) = by['costs']
    assert F == [T, 2 * T, T + 5, T + 7] and pred == [-1, 0, 1, 1] and kind == [0, 1, 2, 3]
    _, (F, pred, kind, paths) = by['costs, value 0']
    assert F == [T, 5, 7] and pred == [-1, -1, -1]                 # T - T is not above 0
    _, (F, pred, kind, paths) = by['staircase of 64']
    assert F[63] == 64 * T - 63 * 16 > 1 << 45 and pred == [-1] + list(range(63)) and paths == [(F[63], list(range(64)))]
    mine, (F, pred, kind, paths) = by['mixed']
    assert len(mine) == 4 and F == [T, 0, T - 13, -1] and pred == [-1, 0, 0, -1] and kind == [0, 1, 2, 0]
    assert paths == [(T, [0]), (-13, [2]), (-T, [1]), (-1, [3])]      # both later walks stop on chain 0: their scores are differences
    rows, n = lc.rows(mine, 15)
    assert n == 4 and all(type(v) is int for row in rows for v in row)           # finite, exact rows


def test_link_range_fuzz_draws_from_both_signs_and_the_bound():
    (small, p_small), (wide, p_wide) = edges.range_fuzz()
    assert len(small) == 100 and len(wide) == 40 and p_small == lcases.FUZZ_SMALL and p_wide == {}
    assert {0, 1, 2, 63, 64} <= {len(mine) for mine in small}
    seen, neg_linked, kinds, top = set(), 0, set(), 0
    for segments, p in edges.range_fuzz():
        for mine in segments:
            seen |= {c['score'] for c in mine}
            F, pred, kind, paths = lc.link(mine, 15, **p)
            neg_linked += sum(1 for c in range(len(mine)) if pred[c] >= 0 and F[c] <= 0)
            kinds |= set(kind)
            top = max([top] + F)
    assert seen == set(edges.RANGE_SCORES) and min(seen) == -edges.TOP and max(seen) == edges.TOP
    assert neg_linked > 50 and kinds == {0, 1, 2, 3} and top > 4 * edges.TOP
    assert lcases.fuzz_segments(5, 20) == lcases.fuzz_segments(5, 20, scores=lcases.FUZZ_SCORES)


def test_link_workgroup_segments_end_with_a_full_segment():
    for nseg in (3, 4, 8, 9):
        segments = edges.workgroup_segments(nseg)
        assert len(segments) == nseg and len(segments[-1]) == 64 and min(c['score'] for c in segments[-1]) < 0
        assert len({len(mine) for mine in segments}) > 1


# ---- K7j -----------------------------------------------------------------------------------------------------------------------------

def test_junction_slides_tie_in_classes_1_2_3_and_the_first_t_wins():
    seen = set()
    for cls, planted, batch in edges.slide_batches():
        contigs, texts = jcases.codes_of(batch)
        rows = jcases.want_rows(batch)
        assert len(batch[2]) == 18
        for t, (slide, a, want), row in zip(batch[2], planted, rows):
            m = t[6] - t[4]
            assert m == 2 * a + slide and cls_of(m) == cls and t[7] == want
            strands = {0: (0, 1), 1: (0,), -1: (1,)}[want]
            top = jc.maxima(contigs[t[2]], texts[t[0]], (t[1],) + tuple(t[3:]), **batch[3])
            assert top == [(s, a + d) for s in strands for d in range(slide + 1)], (cls, slide, want, top)
            assert row[:4] == [0, 2 * m - 12 - 12, strands[0], a] and row[10] == row[11] == 6      # every letter matched; the first t of the tie
            seen.add((cls, slide, t[1], want))
    assert len(seen) == 3 * 3 * 2 * 3


def test_junction_class_fuzz_covers_every_class_at_every_slack():
    counts = collections.Counter()
    ties = 0
    for batch in edges.class_fuzz_batches():
        contigs, texts = jcases.codes_of(batch)
        for t, row in zip(batch[2], jcases.want_rows(batch)):
            m = t[6] - t[4]
            assert 65 <= m <= 512 and row[0] == 0
            counts[(batch[3]['slack'], cls_of(m))] += 1
            top = jc.maxima(contigs[t[2]], texts[t[0]], (t[1],) + tuple(t[3:]), **batch[3])
            assert (row[2], row[3]) == top[0]
            ties += len(top) > 1
    assert sorted(counts) == [(s, c) for s in (0, 5, 64) for c in (1, 2, 3)] and min(counts.values()) >= 8
    assert {t[6] - t[4] for b in edges.class_fuzz_batches() for t in b[2]} >= {65, 128, 129, 256, 257, 512}
    print('class fuzz: %d of %d tasks tie over (strand, t)' % (ties, sum(counts.values())))
    assert ties >= 24


def test_junction_clip_batch_clips_inside_classes_1_2_3():
    batch = edges.clip_batch()
    contigs, texts = jcases.codes_of(batch)
    size = len(contigs[1])
    seen, classes, who = set(), set(), set()
    for t, row in zip(batch[2], jcases.want_rows(batch)):
        m = t[6] - t[4]
        D, A = jc.windows(contigs[1], t[3], t[5], m, batch[3]['slack'])
        assert row[0] == 0 and t[2] == 1 and cls_of(m) >= 1 and len(D) < m and len(A) < m and len(D) == size - t[3] and len(A) == t[5]
        seen.add((len(D), len(A)))
        classes.add(cls_of(m))
        who.add((t[1], t[7]))
    assert {(0, 0)} | {(n, n) for n in edges.CLIPS} | {(0, n) for n in edges.CLIPS} | {(n, 0) for n in edges.CLIPS} <= seen
    assert classes == {1, 2, 3} and who == {(minus, want) for minus in (0, 1) for want in (0, 1, -1)}
    assert 4 in contigs[1] and all(4 in t for t in texts[:2]) and min(len(t) for t in texts) >= 520
    first = jcases.want_rows(batch)[0]
    assert first[4:8] == [0, 0, size, 0] and first[10:12] == [6, 6]       # nD = nA = 0: the neighbours' GT and AG cost `other`


def test_junction_bound_scoring_is_on_the_bound_at_the_full_span():
    p = jc.parameters(edges.BOUND_SCORING)
    donor, acceptor, other = jc.tables(p)
    assert (p['max_span'], p['slack']) == (jc.MAX_SPAN, jc.MAX_SLACK)
    assert (2 * 512 + 64) * 963 + 500 + max(donor + [other]) + max(acceptor + [other]) == (2 * 512 + 64) * 963 + 500 + 165 + 166 == jc.BOUND - 1
    assert jc.admitted(p) is None and jc.admitted(jc.parameters(dict(edges.BOUND_SCORING, intron_open=501))) == -2
    batch = edges.bound_planted((130, 300, 512), seed=53)
    for t, row in zip(batch[2], jcases.want_rows(batch)):
        assert row[0] == 0 and row[1] == row[8] + row[9] - row[10] - row[11] - 500 and max(abs(v) for v in row[8:10]) < jc.BOUND, (t, row)
        assert row[1] > 963 * (t[6] - t[4]) // 2                      # the planted junction is found: most letters match
    batches = edges.bound_batches()
    assert sorted(batches) == ['planted', 'poly', 'unrelated']
    low = 0
    for name, batch in batches.items():
        assert [t[6] - t[4] for t in batch[2]] == list(edges.BOUND_SPANS) and batch[3] == edges.BOUND_SCORING
        contigs, texts = jcases.codes_of(batch)
        for t, row in zip(batch[2], jcases.want_rows(batch)):
            assert row[0] == 0
            if name == 'poly':
                HL, HR, start, end = jc.sides(contigs[0], texts[0], (t[1],) + tuple(t[3:]), p)
                low = min(low, int((HL - start[0][None, :]).min()), int((HR - end[1][None, :]).min()))
                assert row[1] < 0 and int(HL.max()) <= 0 and int(HR.max()) <= 0       # no cell matches
    print('the lowest side score less a site cost: %d of -%d' % (low, jc.BOUND))
    # 512 letters against 576 that match none of them: 512 mismatches and one gap of 64, less the cost of a site that is not canonical.
    # No side score of the definition lies lower at this scoring: the bound of seed_device.h counts every cell of both windows.
    assert low == -(512 * 962 + 963 + 63 * 950 + 165) > -jc.BOUND


# ---- K7c -----------------------------------------------------------------------------------------------------------------------------

def test_circle_full_read_fills_every_slot():
    texts = edges.full_texts()
    for r, minus in ((edges.FULL_READ, 0), (edges.FULL_READ + 1, 1)):
        segs, best, mine, rows = edges.full_tasks(texts[r], 64)
        assert [len(s) for s in segs] == ([0, 64] if minus else [64, 0])
        assert best[0] == minus and len(best[2]) == 64 and len(mine) == 63 == edges.FULL['max_chains'] - 1
        spans = [t[6] - t[4] for t in mine]
        done = [cls_of(m) for m, v in zip(spans, rows) if v[0] == 0]
        assert {cls_of(m) for m in spans if m <= jc.MAX_SPAN} == set(done) == {0, 1, 2, 3} and collections.Counter(v[0] for v in rows) == {0: len(mine) - 1, 1: 1}
        assert sum(1 for m in spans if m > jc.MAX_SPAN) == 1 and sum(1 for m in spans if m <= 64) == len(mine) - len(edges.FULL_JUNK)
        row = edges.full_row(texts[r], 64)
        win = min((o for o, v in enumerate(rows) if v[0] == 0), key=lambda o: (-rows[o][1], o))
        assert row[0] == cc.FOUND and row[9:15] == [minus, best[1], 64, len(mine), len(mine) - 1, win] and 0 < win < len(mine) - 1
    assert edges.full_row(texts[edges.FULL_READ], 64)[1:8] == edges.full_row(texts[edges.FULL_READ + 1], 64)[1:8]
    for max_chains, slots in ((16, 15), (2, 1), (1, 1)):
        segs, best, mine, rows = edges.full_tasks(texts[edges.FULL_READ], max_chains)
        assert len(segs[0]) == max_chains and len(mine) <= slots
    assert edges.full_row(texts[edges.FULL_READ], 16)[0] == cc.FOUND and edges.full_row(texts[edges.FULL_READ], 16)[12] >= 2
    assert edges.full_row(texts[edges.FULL_READ], 2)[0] == edges.full_row(texts[edges.FULL_READ], 1)[0] == cc.NO_BACKSPLICE
    assert edges.full_row(texts[edges.FULL_READ], 64) in edges.expected(edges.middle_batch(), 64)[0][1:-1]


@pytest.mark.parametrize('max_chains', [1, 2, 3, 64])
def test_circle_planted_reads_at_other_strides(max_chains):
    rows, where, tab = ccases.want(max_chains=max_chains)
    base = ccases.want()[0]
    assert len(rows) == len(base) and ccases.want(False, 0) == ccases.want() == ccases.want(max_chains=16)
    for segs in ccases.segments(max_chains):
        assert max(len(s) for s in segs) <= max_chains
    if max_chains == 1:                                 # one chain a segment: no link, so no back-splice
        assert {v[0] for v in rows} == {cc.NO_PATH, cc.NO_BACKSPLICE} and tab == []
        assert [v[0] == cc.NO_PATH for v in rows] == [v[0] == cc.NO_PATH for v in base]
        assert all(v[11:13] == [1, 0] for v in rows if v[0] == cc.NO_BACKSPLICE)
    else:
        assert sum(1 for v in rows if v[0] == cc.FOUND) >= 40 and max(v[12] for v in rows) <= max(max_chains - 1, 1)
    if max_chains == 64:
        assert rows == base                             # no planted read has more than 16 chains a strand


def test_circle_batches_cross_the_workgroups_with_the_statuses_interleaved():
    texts = edges.full_texts()
    assert [n for n, _, _ in edges.BATCHES] == [255, 256, 256, 257, 513]
    for n, hub, last in edges.BATCHES:
        order = edges.cycled(n, hub, last)
        rows, where, tab = edges.expected([texts[r] for r in order])
        statuses = [v[0] for v in rows]
        assert len(order) == n and all(set(statuses[a:a + 16]) == {0, 1, 2, 3} for a in range(n - 16))
        assert edges.FULL_READ in order
        if last:
            assert (statuses[-1] == cc.FOUND) == (last == 'found')
        if hub:                                         # one circle with more than 256 reads, spread over the whole batch
            g = where[0]
            members = [r for r, w in enumerate(where) if w == g]
            assert len(members) > 256 and members[0] == 0 and members[-1] >= n - 2 and max(b - a for a, b in zip(members, members[1:])) <= 4
            assert tab[g][6] == len(members) and tab[g][8] == 0 and tab[g][7] == max(rows[r][7] for r in members) > min(rows[r][7] for r in members)
            assert len(set(edges.hub_reads())) >= 3
    assert edges.full_row(texts[edges.FULL_READ])[12] >= 2 and set(edges.by_status()) == {0, 1, 2, 3} and min(len(v) for v in edges.by_status().values()) >= 1


def test_circle_far_world_sorts_contig_first_with_starts_above_65536():
    contigs, circles, reads = edges.far_world()
    genome, (rows, where, tab) = edges.far_want()
    assert sum(len(t) for _, t in contigs) <= 80000 and len(contigs[0][1]) > 65536 + 3000
    for (label, _), v, w in zip(reads, rows, where):
        if label is None:
            assert v[0] != cc.FOUND and w == -1
        else:
            assert v[0] == cc.FOUND and tuple(v[1:4]) == circles[label] and (v[5], v[6]) == (13, 2), (label, v)     # to the base, GT-AG
    assert circles['short'][1] == circles['long'][1] > 65536 and circles['short'][2] < circles['long'][2] and circles['low'][1] < 256
    assert [tuple(t[:3]) for t in tab] == [circles[name] for name in ('short', 'long', 'near', 'low')]       # contig first, whatever the starts
    starts = [t[1] for t in tab]
    assert starts != sorted(starts) and [t[6] for t in tab] == [3, 2, 2, 2]
    assert [t[8] for t in tab] == [3, 1, 2, 0] and {v[9] for v in rows if v[0] == cc.FOUND} == {0, 1}
    assert where[:4] == [3, 1, 2, 0]                    # the reads come in another order than the table's


def test_circle_share_batch_and_the_greedy_cut():
    order = edges.share_batch()
    assert order[9] == edges.FULL_READ and len(order) == 19 and len(set(order)) == 19
    assert edges.greedy_shares([0, 5, 9, 30, 34, 34, 40], 21) == [(0, 2), (2, 3), (3, 6)]
