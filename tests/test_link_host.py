"""K7's link step on the CPU: the checker tests/link_check.py against an independent statement (every chain subsequence enumerated), the
partition of the kinds, the tie rules, and the planted cases of tests/link_cases.py asserted with seed_check and the checker alone,
before tests/test_gpu_link.py asks the GPU about the same cases; and the __host__ __device__ link functions of csrc/seed_device.h
against the checker: tests/link_host.hip is a program of its own, built with AddressSanitizer and UBSan linked into it alone, that
prints its inputs and answers.  No GPU is touched."""
import itertools
import os
import random
import re
import shutil
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import link_cases as cases  # noqa: E402
import link_check as lc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which('hipcc') or ('/opt/rocm/bin/hipcc' if os.path.exists('/opt/rocm/bin/hipcc') else None)


def test_f_equals_the_best_of_all_chain_subsequences():
    """F of a chain is the greatest total, scores plus link terms, over every subsequence of the chains, taken in rank order with every
    consecutive link admissible, that ends in it"""
    rng = random.Random(17)
    linked = 0
    segments = [(mine, cases.FUZZ_SMALL) for mine in cases.fuzz_segments(1000, 300, most=7)] + [(mine, {}) for mine in cases.fuzz_segments(1001, 100, most=7, wide=True)]
    for t, (mine, p) in enumerate(segments):
        k = rng.choice((4, 15, 28))
        F, pred, kind, paths = lc.link(mine, k, **p)
        rank, order = lc.ranks(mine)
        best = {}
        for size in range(1, len(mine) + 1):
            for sub in itertools.combinations(order, size):
                total = mine[sub[0]]['score']
                for j, i in zip(sub, sub[1:]):
                    term = lc.link_term(mine[j], mine[i], k, lc.parameters(p))
                    if term is None:
                        total = None
                        break
                    total += term[0] + mine[i]['score']
                if total is not None:
                    best[sub[-1]] = max(best.get(sub[-1], total), total)
        assert F == [best[c] for c in range(len(mine))], (t, mine)
        for c in range(len(mine)):
            assert (pred[c] == -1) == (kind[c] == 0)
            if pred[c] >= 0:
                linked += 1
                term = lc.link_term(mine[pred[c]], mine[c], k, lc.parameters(p))
                assert rank[pred[c]] < rank[c] and term[1] == kind[c] and F[c] == mine[c]['score'] + F[pred[c]] + term[0] > mine[c]['score']
        assert sorted(c for _, walk in paths for c in walk) == list(range(len(mine)))       # every chain in exactly one path
    assert linked > 200


def test_kinds_partition_the_skew():
    """for every d of a swept range and every span, exactly one kind or none (classify asserts the 'at most one'), and each where it belongs"""
    p = lc.parameters(dict(max_skew=7, max_intron=19, max_circle=11))
    seen = set()
    for d in range(-40, 41):
        for span in range(-3, 15):
            kind = lc.classify(d, span, p)
            seen.add(kind)
            assert kind == (1 if abs(d) <= 7 else 2 if 7 < d <= 19 else 3 if d < -7 and 0 < span <= 11 else 0)
    assert seen == {0, 1, 2, 3}
    p = lc.parameters(dict(max_skew=0, max_intron=0, max_circle=0))
    assert [lc.classify(d, 5, p) for d in (-1, 0, 1)] == [0, 1, 0]


def test_thresholds_as_planted():
    for label, mine, p, want in cases.threshold_cases():
        F, pred, kind, paths = lc.link(mine, 15, **p)
        assert (kind[1], pred[1]) == (want, 0 if want else -1), label
        assert len(paths) == (1 if want else 2), label
    by = {label: lc.link(mine, 15, **p) for label, mine, p, _ in cases.threshold_cases()}
    assert by['a value of exactly 1'][0] == [17, 81] and by['a value of exactly 0'][0] == [16, 80]
    assert by['overlap paid once: value 1'][0] == [21, 81]
    assert by['q = -32'][0][1] == 80 + 100 - 32             # the overlap is paid once, and beta(0) is 0


def test_tie_rules_as_planted():
    mine, want = cases.order_case()
    assert lc.ranks(mine)[0] == want
    for flip in (False, True):
        mine, winner = cases.equal_candidates_case(flip)
        F, pred, kind, paths = lc.link(mine, 15)
        rank, _ = lc.ranks(mine)
        assert F[0] == F[1] == 100 and pred[2] == winner and rank[winner] == 1 and F[2] == 150
    mine = cases.equal_f_case()
    F, pred, kind, paths = lc.link(mine, 15)
    assert F == [70, 70] and lc.ranks(mine)[0] == [1, 0] and paths == [(70, [1]), (70, [0])]


def test_path_shapes_as_planted():
    F, pred, kind, paths = lc.link(cases.shared_predecessor_case(), 15)
    assert pred == [-1, 0, 0] and kind == [0, 1, 2] and F == [100, 190, 134]
    assert paths == [(190, [0, 1]), (34, [2])]               # the second walk stops on chain 0, already used: its score is the difference
    F, pred, kind, paths = lc.link(cases.staircase_case(), 15)
    assert pred == [-1] + list(range(63)) and set(kind[1:]) == {2} and paths == [(F[63], list(range(64)))] and F[63] == 64 * 50 - 63 * 16
    F, pred, kind, paths = lc.link(cases.isolated_case(), 15)
    assert pred == [-1] * 64 and len(paths) == 64 and all(len(walk) == 1 for _, walk in paths)
    assert [score for score, _ in paths] == sorted((40 + t % 3 for t in range(64)), reverse=True)


def test_fuzz_segments_are_rich_in_ties_and_kinds():
    kinds, tied, linked = set(), 0, 0
    for wide, count, p in ((False, 300, cases.FUZZ_SMALL), (True, 75, {})):
        segments = cases.fuzz_segments(5, count, wide=wide)
        assert {0, 1, 2, 63, 64} <= {len(mine) for mine in segments}
        for mine in segments:
            F, pred, kind, paths = lc.link(mine, 15, **p)
            kinds |= set(kind)
            tied += len(F) - len(set(F))
            linked += sum(1 for v in pred if v >= 0)
    assert kinds == {0, 1, 2, 3} and tied > 1000 and linked > 3000


def test_planted_world_is_what_the_issue_asks_for():
    contigs, genes = cases.world()
    assert len(contigs) == 3 and sum(len(t) for _, t in contigs) <= 40000 and len(genes) == 5
    text = dict(contigs)
    for name, strand, exons in genes:
        assert 2 <= len(exons) <= 5 and all(120 <= b - a <= 400 for a, b in exons)
        for (_, b), (a, _) in zip(exons, exons[1:]):
            assert 600 <= a - b <= 3000 and (text[name][b:b + 2], text[name][a - 2:a]) == (('GT', 'AG') if strand == '+' else ('CT', 'AC'))
    reads = cases.reads()
    assert {(r['what'], r['errors'], r['minus']) for r in reads} >= {('circle', False, False), ('circle', False, True), ('circle', True, False),
                                                                     ('circle', True, True), ('linear', False, False), ('linear', False, True)}


def test_planted_reads_carry_the_truth_in_the_checker():
    """error-free reads: the best path holds every chain of its strand, has one back-splice for a circle and none for a linear read, each
    exon is one chain, and the circle's ends lie within w - 1 letters of the planted circle's first and last base: inside by the winnowing
    guarantee (a window of w k-mers wholly inside a shared stretch has its minimum selected in both sequences), outside only as far as the
    letters behind the junction happen to continue the exon"""
    genome, idx, paths = cases.checked()
    asserted = 0
    for r, (read, mine) in enumerate(zip(cases.reads(), paths)):
        assert mine, r
        if read['errors']:
            continue
        asserted += 1
        best = mine[0]
        segs = lc.segment_chains(genome, idx, lc.sc.encode(read['text']), cases.K, cases.W, cases.MAX_OCC)
        assert (best['contig'], best['minus']) == (read['contig'], read['minus']), r
        assert len(best['chains']) == len(segs[int(read['minus'])]) and not segs[1 - int(read['minus'])], r
        want = cases.expected_pieces(read)
        links = []
        for t, piece in enumerate(want):                     # an intron between the exons of a piece, one back-splice between the two pieces
            links += (['backsplice'] if t else []) + ['intron'] * (len(piece) - 1)
        assert best['links'] == links and len(want) == (2 if read['what'] == 'circle' else 1), (r, best['links'], links)
        assert len(best['chains']) == sum(len(p) for p in want), r
        first, last = read['exons'][0][0], read['exons'][-1][1] - 1
        if read['what'] == 'circle':
            ctg, a, b = best['circle']
            assert ctg == read['contig'] and abs(a - first) <= cases.W - 1 and abs(last - (b - 1)) <= cases.W - 1, (r, best['circle'], first, last)
            assert 'rotation' in best and len(best['pieces']) == 2, r
        else:
            assert 'circle' not in best and 'rotation' not in best and len(best['pieces']) == 1, r
        for piece, exons in zip(best['pieces'], want):      # the anchors bound a piece inside its planted exons, within w - 1 of a whole end
            lo, hi = exons[0][0], exons[-1][1]
            assert lo is None or abs(piece['ref_start'] - lo) <= cases.W - 1, r
            assert hi is None or abs(hi - (piece['ref_end'] - 1)) <= cases.W - 1, r
    assert asserted == 20


def test_rotation_is_where_the_back_splice_target_begins():
    """read along the contig's strand, the circle's first exon begins `junction` letters into the read: the rotation is its first anchor"""
    genome, idx, paths = cases.checked()
    for r, (read, mine) in enumerate(zip(cases.reads(), paths)):
        if read['errors'] or read['what'] != 'circle':
            continue
        got = mine[0]['rotation']
        along = len(read['text']) - got if read['minus'] else got
        assert abs(along - read['junction']) <= cases.W - 1, (r, got, read['junction'])


def test_link_chains_of_the_checkers_own_chains_gives_link_reads():
    genome, idx, paths = cases.checked()
    reads = cases.reads()
    lists = []
    for read in reads:
        segs = lc.segment_chains(genome, idx, lc.sc.encode(read['text']), cases.K, cases.W, cases.MAX_OCC)
        lists.append([lc.map_style(genome.names, c, len(read['text']), cases.K) for seg in segs for c in seg])
    assert lc.link_chains(genome.names, lists, [len(r['text']) for r in reads], cases.K) == paths


@pytest.mark.skipif(HIPCC is None, reason='hipcc is not installed')
def test_device_header_link_functions_equal_the_checker_under_sanitizers(tmp_path):
    exe = str(tmp_path / 'link_host')
    build = subprocess.run([HIPCC, '--offload-arch=gfx950', '-std=c++17', '-O1', '-g', '-Xarch_host', '-fsanitize=address,undefined',
                            '-I', os.path.join(ROOT, 'ciri_long_amd', 'csrc'), os.path.join(ROOT, 'tests', 'link_host.hip'), '-o', exe],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run(['timeout', '-k', '10', '120', exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert 'runtime error' not in run.stderr, run.stderr              # UBSan reports and goes on
    lines = run.stdout.splitlines()
    m = re.match(r'^link_host: (\d+) lines: ok$', lines[-1])
    assert m and int(m.group(1)) == len(lines) - 1, lines[-1]
    names = ('max_query_gap', 'max_overlap', 'max_skew', 'max_intron', 'max_circle', 'intron_cost', 'backsplice_cost')

    def chain(v):
        return cases.chain(v[0], v[1], v[2], v[3], v[4], v[5])
    counts = {'link': 0, 'before': 0}
    kinds = {0: 0, 1: 0, 2: 0, 3: 0}
    for line in lines[:-1]:
        t = line.split(' ')
        counts[t[0]] += 1
        if t[0] == 'link':
            v = [int(x) for x in t[1:21]]
            want = lc.link_term(chain(v[8:14]), chain(v[14:20]), v[0], dict(zip(names, v[1:8])))
            assert (t[22], int(t[21])) == (('none', 0) if want is None else (str(want[0]), want[1])), line
            kinds[int(t[21])] += 1
        else:
            v = [int(x) for x in t[1:]]
            a, ca, b, cb = chain(v[0:6]), v[6], chain(v[7:13]), v[13]
            assert v[14] == int(lc.key([a], 0)[:3] + (ca,) < lc.key([b], 0)[:3] + (cb,)), line
    assert counts['link'] > 3200 and counts['before'] == 3400 and min(kinds.values()) > 100, (counts, kinds)
