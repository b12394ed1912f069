"""K7c on the CPU: the checker tests/circle_check.py (best path, tasks, winner, flank codes, rows, table) held to what already exists --
junction_check.circle_of over the refined paths of link_check, which restate seed.call_circles -- on the planted reads of
tests/circle_cases.py; the proof, from the checkers alone, that the planted set holds every case tests/test_gpu_circles.py then asks the
GPU about; and the __host__ __device__ selection functions of csrc/seed_device.h against the checker: tests/circle_host.hip is a
program of its own, built with AddressSanitizer and UBSan linked into it alone.  No GPU is touched."""
import collections
import os
import re
import shutil
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import circle_cases as cases  # noqa: E402
import circle_check as cc  # noqa: E402
import junction_check as jc  # noqa: E402
import link_check as lc  # noqa: E402
import seed_check as sc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which('hipcc') or ('/opt/rocm/bin/hipcc' if os.path.exists('/opt/rocm/bin/hipcc') else None)


def composed(scoring=False):
    """what seed.call_circles gives per read, without its path, by the checkers that restate it"""
    out = []
    for mine in cases.refined(scoring):
        got = jc.circle_of(mine[0]) if mine else None
        out.append({k: v for k, v in got.items() if k != 'path'} if got else None)
    return out


def row_of(name, scoring=False):
    return cases.want(scoring)[0][cases.label(name)]


@pytest.mark.parametrize('scoring', [False, True])
def test_checker_rows_equal_the_composed_route_field_for_field(scoring):
    genome = cases.checked()[0]
    rows, _, _ = cases.want(scoring)
    want = composed(scoring)
    assert len(rows) == len(want) == len(cases.reads())
    for r, (v, w) in enumerate(zip(rows, want)):
        assert cc.circle_dict(genome, v) == w, (r, cases.reads()[r][0], v, w)
        assert len(v) == cc.ROW and v[15] == 0
        if v[0] == cc.NO_PATH:
            assert v[1:] == [0] * 15 and not cases.refined(scoring)[r]
        else:
            best = cases.refined(scoring)[r][0]
            assert v[9:14] == [int(best['minus']), best['score'], len(best['chains']), best['links'].count('backsplice'),
                               sum(1 for j in best['junctions'] if j['status'] == 0)], r
            assert v[0] != cc.FOUND or best['junctions'][v[14]]['score'] == v[7]
            assert v[0] == cc.FOUND or v[1:9] == [0] * 8 and v[14] == 0


@pytest.mark.parametrize('scoring', [False, True])
def test_table_equals_a_counter_over_the_answers(scoring):
    genome = cases.checked()[0]
    rows, where, tab = cases.want(scoring)
    want = composed(scoring)
    count = collections.Counter((w['contig'], w['start'], w['end'], w['strand']) for w in want if w)
    listed = cc.table_dicts(genome, tab)
    assert [(t['contig'], t['start'], t['end'], t['strand']) for t in listed] == sorted(count, key=lambda key: (genome.names.index(key[0]),) + key[1:3] + ('+-'.index(key[3]),))
    for g, t in enumerate(listed):
        members = [r for r, w in enumerate(want) if w and (w['contig'], w['start'], w['end'], w['strand']) == (t['contig'], t['start'], t['end'], t['strand'])]
        assert t['reads'] == count[(t['contig'], t['start'], t['end'], t['strand'])] == len(members)
        assert t['score'] == max(want[r]['score'] for r in members) and t['first_read'] == members[0]
        assert {want[r]['signal'] for r in members} == {t['signal']} and t['circ_id'] == want[members[0]]['circ_id']
        assert [where[r] for r in members] == [g] * len(members)
    assert [g for g, w in zip(where, want) if not w] == [-1] * sum(1 for w in want if not w)


def test_min_path_score_above_some_paths_scores():
    genome, idx, _ = cases.checked()
    scores = sorted(v[10] for v in cases.want()[0] if v[0] != cc.NO_PATH)
    bar = 200
    assert scores[0] < bar < scores[-1]
    rows, _, _ = cases.want(False, bar)
    changed = 0
    for r, (text, v) in enumerate(zip(cases.texts(), rows)):
        paths = lc.link_read(genome, idx, sc.encode(text), cases.K, cases.W, cases.MAX_OCC, min_path_score=bar, **dict(cases.LINK))
        got = jc.circle_of(jc.refine_paths(genome, sc.encode(text), paths[:1], cases.K)[0]) if paths else None
        assert cc.circle_dict(genome, v) == ({k: x for k, x in got.items() if k != 'path'} if got else None), r
        changed += v != cases.want()[0][r]
    assert changed >= 5


def test_planted_reads_hold_every_status_and_every_named_case():
    genome, _, paths = cases.checked()
    rows, where, tab = cases.want()
    assert {v[0] for v in rows} == {0, 1, 2, 3}
    assert row_of('empty')[0] == row_of('random')[0] == cc.NO_PATH and row_of('linear')[0] == row_of('linear minus')[0] == cc.NO_BACKSPLICE
    # the best path has no back-splice while a lower path has one: the answer stays status 2, as call_circles answers None
    mine = paths[cases.label('linear above circle')]
    assert 'backsplice' not in mine[0]['links'] and any('backsplice' in p['links'] for p in mine[1:]) and mine[0]['score'] > mine[1]['score']
    assert row_of('linear above circle')[0] == cc.NO_BACKSPLICE and composed()[cases.label('linear above circle')] is None
    # two reads whose strands tie on score (a read that is its own reverse complement gives both segments the same chains): minus decides
    _, link_p, _ = cc.split(cases.LINK)
    for name in ('palindrome a', 'palindrome b'):
        segs = cases.segments()[cases.label(name)]
        plus, minus = cc.best_path([segs[0], []], cases.K, 0, **link_p), cc.best_path([[], segs[1]], cases.K, 0, **link_p)
        assert plus[1] == minus[1] and segs[0][plus[2][0]]['x_first'] == segs[1][minus[2][0]]['x_first'] and (plus[0], minus[0]) == (0, 1)
        assert row_of(name)[0] == cc.FOUND and row_of(name)[9] == 0 and row_of(name)[10] == plus[1]
    # two back-splice links in one path: equal J, the first wins; different J, the greater wins although it is the second
    for name, winner in (('two turns equal', 0), ('two turns second wins', 1)):
        (a, b) = cases.refined()[cases.label(name)][0]['junctions']
        assert a['status'] == b['status'] == 0 and (a['score'] == b['score'] if winner == 0 else a['score'] < b['score'])
        v = row_of(name)
        assert v[12:15] == [2, 2, winner] and v[7] == (a, b)[winner]['score'] and v[8] == (a, b)[winner]['read_pos']
    # more than max_span letters between the anchors: status 3, at the default max_span and, for many more, at SCORING's 40
    v = row_of('too wide')
    assert v[0] == cc.NO_JUNCTION and v[12:14] == [1, 0] and [j['status'] for j in cases.refined()[cases.label('too wide')][0]['junctions']] == [1]
    low = cases.want(True)[0]
    assert sum(1 for a, b in zip(rows, low) if a[0] == cc.FOUND and b[0] == cc.NO_JUNCTION) >= 20 and {b[0] for b in low} == {0, 1, 2, 3}
    # a circle that ends with its contig, one that begins it: flank code -1
    v = row_of('contig end')
    assert v[0] == 0 and v[3] == len(genome.codes[v[1]]) and v[5] == -1 and v[6] == 2 and composed()[cases.label('contig end')]['signal'] == '-AG'
    v = row_of('contig start')
    assert v[0] == 0 and v[2] == 0 and v[6] == -1 and v[5] == 13 and composed()[cases.label('contig start')]['signal'] == 'GT-'
    # code 4 and lower-case letters in a flank
    v = row_of('n and lower case')
    text = dict(cases.world()[0])[genome.names[v[1]]]
    assert v[0] == 0 and (text[v[3]:v[3] + 2], text[v[2] - 2:v[2]]) == ('GN', 'ag') and (v[5], v[6]) == (5 * 2 + 4, 5 * 0 + 2)
    assert composed()[cases.label('n and lower case')]['signal'] == 'GN-AG'
    # one circle supported by reads given on both strands: one table row with reads == 2
    a, b = row_of('n and lower case'), row_of('n and lower case minus')
    assert a[1:8] == b[1:8] and (a[9], b[9]) == (0, 1) and where[cases.label('n and lower case')] == where[cases.label('n and lower case minus')]
    assert tab[where[cases.label('n and lower case')]][6] == 2
    # the junction widths around K7j's class bound
    widths = set()
    for r, segs in enumerate(cases.segments()):
        best = cc.best_path(segs, cases.K, 0, **link_p)
        if best:
            widths |= {t[6] - t[4] for t in cc.tasks(r, best[0], segs[best[0]], best[2], best[3], cases.K)}
    assert {63, 64, 65} <= widths and max(widths) > jc.MAX_SPAN


def test_one_pair_of_coordinates_on_both_transcript_strands_is_two_table_rows():
    """On ONE contig this cannot be planted, at any scoring: both strands of a task see the same HL and HR, so at a given (start, end)
    J+ and J- differ by the site costs of that place alone.  A read answered (start, end, -) has J-(start, end) > J+ everywhere, so
    cost- < cost+ there; a read answered (start, end, +) has J+(start, end) >= J-(start, end), so cost+ <= cost-: both cannot hold.
    The pair is planted on two contigs of one layout (AG..GT around the one, AC..CT around the other); that the strand is part of the
    table's key on one contig is asserted on rows written by hand."""
    rows, where, tab = cases.want()
    a, b = rows[cases.label('plus transcript')], rows[cases.label('minus transcript')]
    assert a[0] == b[0] == 0 and a[2:4] == b[2:4] and (a[4], b[4]) == (0, 1) and (a[5], a[6]) == (b[5], b[6]) == (13, 2)
    ta, tb = tab[where[cases.label('plus transcript')]], tab[where[cases.label('minus transcript')]]
    assert ta[1:3] == tb[1:3] and (ta[3], tb[3]) == (0, 1) and where[cases.label('plus transcript')] != where[cases.label('minus transcript')]
    by_hand = [[0, 3, 10, 90, 1, 13, 2, 7, 5] + [0] * 7, [2] + [0] * 15, [0, 3, 10, 90, 0, 13, 2, 9, 5] + [0] * 7, [0, 3, 10, 90, 1, 13, 2, 11, 6] + [0] * 7,
               [0, 2, 10, 90, 1, 13, 2, 1, 5] + [0] * 7, [0, 3, 9, 91, 0, 13, 2, 1, 5] + [0] * 7]
    t, w = cc.table(by_hand)
    assert t == [[2, 10, 90, 1, 13, 2, 1, 1, 4, 0], [3, 9, 91, 0, 13, 2, 1, 1, 5, 0], [3, 10, 90, 0, 13, 2, 1, 9, 2, 0], [3, 10, 90, 1, 13, 2, 2, 11, 0, 0]]
    assert w == [3, -1, 2, 3, 0, 1]


def host_input(scoring, min_path_score):
    """the planted segments as tests/circle_host.hip reads them, and per read the checker's tasks"""
    genome = cases.checked()[0]
    text_of = cases.world()[0]
    _, link_p, junction_p = cc.split(dict(cases.LINK, **(cases.SCORING if scoring else {})))
    p = jc.parameters(junction_p)
    out = [cases.K, min_path_score, p['max_span'], len(text_of)]
    for (_, text), codes in zip(text_of, genome.codes):
        out += [len(codes)] + [c + (8 if ch.islower() else 0) + (16 if c == 4 else 0) for c, ch in zip(codes, text)]      # bits above the code: dropped
    out.append(len(cases.reads()))
    tasks = []
    for r, (text, segs) in enumerate(zip(cases.texts(), cases.segments())):
        read = sc.encode(text)
        out += [len(read), len(segs[0]), len(segs[1])]
        for minus, mine in enumerate(segs):
            for c in mine:
                out += [r, minus, c['contig'], c['score'], c['anchors'], c['x_first'], c['y_first'], c['x_end'], c['y_end'], 0]
        for mine in segs:
            for v in lc.rows(mine, cases.K, **link_p)[0]:
                out += v
        best = cc.best_path(segs, cases.K, min_path_score, **link_p)
        mine = cc.tasks(r, best[0], segs[best[0]], best[2], best[3], cases.K) if best else []
        tasks.append((best, mine))
        out.append(len(mine))
        for t in mine:
            out += jc.refine(genome.codes[t[2]], read, (t[1],) + tuple(t[3:]), **junction_p)
    return ' '.join(str(int(v)) for v in out) + '\n', tasks


@pytest.mark.skipif(HIPCC is None, reason='hipcc is not installed')
def test_device_header_selection_functions_equal_the_checker_under_sanitizers(tmp_path):
    exe = str(tmp_path / 'circle_host')
    build = subprocess.run([HIPCC, '--offload-arch=gfx950', '-std=c++17', '-O1', '-g', '-Xarch_host', '-fsanitize=address,undefined',
                            '-I', os.path.join(ROOT, 'ciri_long_amd', 'csrc'), os.path.join(ROOT, 'tests', 'circle_host.hip'), '-o', exe],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stdout + build.stderr
    genome = cases.checked()[0]
    for scoring, bar in ((False, 0), (True, 0), (False, 200)):
        text, tasks = host_input(scoring, bar)
        path = str(tmp_path / ('segments_%d_%d.txt' % (scoring, bar)))
        with open(path, 'w') as f:
            f.write(text)
        run = subprocess.run(['timeout', '-k', '10', '120', exe, path], capture_output=True, text=True)
        assert run.returncode == 0, run.stdout + run.stderr
        assert 'runtime error' not in run.stderr, run.stderr          # UBSan reports and goes on
        lines = run.stdout.splitlines()
        m = re.match(r'^circle_host: (\d+) lines: ok$', lines[-1])
        assert m and int(m.group(1)) == len(lines) - 1, lines[-1]
        want_rows = cases.want(scoring, bar)[0]
        p = jc.parameters(cc.split(dict(cases.LINK, **(cases.SCORING if scoring else {})))[2])
        seen = collections.Counter()
        got_tasks = collections.defaultdict(list)
        for line in lines[:-1]:
            t = line.split(' ')
            seen[t[0]] += 1
            if t[0] == 'path':
                best = tasks[int(t[1])][0]
                if best is None:
                    assert t[2] == 'none', line
                else:
                    assert [int(x) for x in t[2:4]] == [best[0], best[1]] and [int(x) for x in t[5:7]] == [len(best[2]), len(tasks[int(t[1])][1])], line
            elif t[0] == 'task':
                v = [int(x) for x in t[1:]]
                got_tasks[v[0]].append(tuple(v[:8]))
                st = jc.status(v[3], v[4], v[5], v[6], p['max_span'])
                assert v[8:] == [1, st, 0 if st else [b for b in range(4) if v[6] - v[4] <= 64 << b][0]], line
            elif t[0] == 'row':
                v = [int(x) for x in t[1:]]
                assert v[1:] == want_rows[v[0]], (line, want_rows[v[0]])
            elif t[0] == 'before':
                sa, ma, xa, pa, got = (int(x) for x in t[1:])
                assert got == int((-sa, ma, xa, pa) < (0, 1, 0, 63)), line
            else:
                assert t[0] == 'revcomp'
                code, got = int(t[1]), int(t[2])
                assert got == cc.revcomp_code(code) and (code < 0 or [got // 5, got % 5] == sc.revcomp([code // 5, code % 5])), line
        assert seen['row'] == seen['path'] == len(want_rows) and seen['before'] == 24 and seen['revcomp'] == 26
        for r, (_, mine) in enumerate(tasks):
            assert got_tasks.get(r, []) == [tuple(t) for t in mine], r
        assert seen['task'] == sum(len(mine) for _, mine in tasks) > 40
    assert any(ch.islower() for _, text in cases.world()[0] for ch in text) and 4 in genome.codes[genome.names.index('n0')]       # bytes above 7 were given
