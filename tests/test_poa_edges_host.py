"""CPU statements to tests/poa_edges.py: the constants are the ones ccs_poa.hip states, every case reaches the edge it is named for
-- read off the oracle's shape record (oracle_lib.oracle_poa_shape: in-degrees, aligned sets, weights, rank distances, end cells,
runs), never off the kernel --, the row formulation the kernel implements (tools/poa_model.py) equals the oracle on the cases it can
run within about a second, and the sets have teeth: one-line faults planted in the model's source are each caught by a named set.

A case that misses its edge fails here; it does not become a weaker GPU test."""
import os
import sys

import numpy as np
import pytest

import oracle_lib
import poa_edges as E

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
import poa_model  # noqa: E402

K = E.constants()
MODEL_CELLS = 1200000           # rows x columns, summed over the sequences of a case: about a second of the model
SET_CELLS = 4000000             # ... and over the cases of a set that the model is held to the oracle on (see model_subset)

_cases, _want, _shape = {}, {}, {}


def cases_of(name):
    if name not in _cases:
        _cases[name] = E.SETS[name](K)
        assert _cases[name], name
    return _cases[name]


def _key(seqs, algorithm, scores, mc=0):
    return (tuple(seqs), algorithm, scores, mc)


def want_of(case):
    """the oracle's (consensus, msa rows, scores), computed once and shared"""
    k = _key(case.seqs, case.algorithm, case.scores, case.min_coverage)
    if k not in _want:
        _want[k] = oracle_lib.oracle_poa(case.seqs, case.algorithm, True, *case.scores, with_scores=True, min_coverage=case.min_coverage)
    return _want[k]


def shape_of(seqs, algorithm, scores):
    k = _key(seqs, algorithm, scores)
    if k not in _shape:
        _shape[k] = oracle_lib.oracle_poa_shape(seqs, algorithm, *scores)
        assert _shape[k] is not None
    return _shape[k]


def shape(case):
    return shape_of(case.seqs, case.algorithm, case.scores)


# ----------------------------------------------------------------------------------------------------------------------------
# the constants and the oracle's shape record
# ----------------------------------------------------------------------------------------------------------------------------
def test_constants_are_parsed_from_the_kernel_source_and_a_missing_one_is_an_error(tmp_path):
    for name in E._PARSED + E._DERIVED:
        assert isinstance(K[name], int) and K[name] > 0, name
    assert K['POA_LDS_BYTES'] == 1024 * K['POA_LDS_KB'] and K['POA_BAND'] == K['POA_BAND_W'] and K['W'] == 128 * K['POA_MAXCP']
    assert K['BT_DRIFT'] == K['BT_W'] // 2 - 4 and K['POA_LDS_SCORES'] == K['POA_LDS_BYTES'] // 4 - 1
    assert sorted(K['RING']) == list(range(1, K['POA_MAXCP'] + 1))
    for cp, ring in K['RING'].items():           # the largest power of two up to 16 whose rows fit the LDS block
        assert ring & (ring - 1) == 0 and ring * (512 * cp + 4) <= K['POA_LDS_BYTES'] and (ring == 16 or 2 * ring * (512 * cp + 4) > K['POA_LDS_BYTES'])
    with open(E.SOURCE) as f:
        src = f.read()
    # the sets follow the file: another register count moves the passes and drops a ring; a smaller LDS block moves the derived ones
    moved = tmp_path / 'moved.hip'
    moved.write_text(src.replace('#define POA_MAXCP %d' % K['POA_MAXCP'], '#define POA_MAXCP 2').replace('#define POA_LDS_KB %d' % K['POA_LDS_KB'], '#define POA_LDS_KB 8'))
    K2 = E.constants(str(moved))
    assert K2['W'] == 256 and sorted(K2['RING']) == [1, 2] and K2['POA_SORT_LDS'] == 8192 // 10 - 2 and K2['BT_W'] == 20 and K2['BT_DRIFT'] == 6
    assert max(E.pass_lengths(K2)) == 513 and max(c.what['cp'] for c in E.source_distance(K2)) == 2
    for gone in ('POA_OVF_CAP = ', '#define POA_BAND_W ', 'int ring = '):
        assert gone in src
        broken = tmp_path / 'broken.hip'
        broken.write_text(src.replace(gone, gone.replace('O', '0').replace('ring', 'rnig')))
        with pytest.raises((KeyError, ValueError)):
            E.constants(str(broken))


def test_the_shape_record_on_a_graph_small_enough_to_check_by_hand():
    # ACGTACGT, then the same without GTA (one edge over three ranks), then with T for the second A (an aligned pair)
    seqs = ['ACGTACGT', 'ACCGT', 'ACGTTCGT', '']
    sh = oracle_lib.oracle_poa_shape(seqs, 1, *E.REF)
    cons, msa, scores, order = oracle_lib.oracle_poa(seqs, 1, True, *E.REF, with_scores=True, with_order=True)
    assert msa == ['ACGTACGT', 'AC---CGT', 'ACGTTCGT'] and len(order) == 9
    # ranks: A C G T (A T) C G T; the second C is entered from A, from the first C (over the deletion: 5 ranks) and from T
    assert list(sh['indeg']) == [0, 1, 1, 1, 1, 1, 3, 1, 1] and list(sh['aligned']) == [1, 1, 1, 1, 2, 2, 1, 1, 1]
    assert list(sh['weight']) == [0, 6, 4, 4, 2, 2, 2, 6, 6] and list(sh['dist']) == [0, 1, 1, 1, 1, 2, 5, 1, 1]
    # end cells in the ranks of the graph the sequence met (8 nodes both times)
    assert sh['end'] == [(0, 0), (8, 5), (8, 8), (0, 0)] and list(sh['hrun']) == [0, 0, 0, 0] and list(sh['vrun']) == [0, 3, 0, 0]
    # an insertion is a horizontal run; local mode ends where the score peaks
    sh = oracle_lib.oracle_poa_shape(['ACGTACGT', 'ACGTNNACGT'], 1, *E.REF)
    assert list(sh['hrun']) == [0, 2] and sh['end'][1] == (8, 10) and sorted(sh['dist'])[-1] == 3
    sh = oracle_lib.oracle_poa_shape(['ACGTACGT', 'TTACGTAAA'], 0, *E.REF)
    assert sh['end'][1] == (5, 7)
    # the entry adds nothing to what oracle_poa answers
    assert oracle_lib.oracle_poa(seqs, 1, True, *E.REF, with_scores=True) == (cons, msa, scores)


# ----------------------------------------------------------------------------------------------------------------------------
# the sets prove their own edges
# ----------------------------------------------------------------------------------------------------------------------------
def test_pass_widths_every_length_in_every_mode_and_a_substitution_at_both_ends_of_every_pass():
    C, W = K['C'], K['W']
    cases = cases_of('pass widths')
    want_len = {C - 1, C, C + 1, 2 * C - 1, 2 * C, 2 * C + 1, W - 1, W, W + 1, W + C, W + C + 1, 2 * W, 2 * W + 1}
    assert {c.algorithm for c in cases} == {0, 1, 2}
    assert any(c.algorithm == 0 and min(c.scores[1:]) < 0 and max(c.scores[1:]) >= 0 for c in cases)       # not the SIMPLE pass
    assert any(c.scores == E.REF for c in cases) and any(c.scores[2] > c.scores[4] and c.scores[3] < c.scores[5] and c.scores != E.REF for c in cases)
    for mode, scores in E.PASS_MODES:
        mine = [c for c in cases if (c.algorithm, c.scores) == (mode, scores)]
        assert {c.what['length'] for c in mine} == want_len
        for c in mine:
            L = c.what['length']
            t, sub, ins, part = c.seqs
            assert (len(t), len(sub), len(ins), len(part)) == (L, L, L + 1, 2 * L // 3)
            diff = [p for p in range(L) if t[p] != sub[p]]
            assert diff == sorted(set(list(range(0, L, W)) + list(range(W - 1, L, W)) + [L - 1]))
            assert ins.replace(E.PRIVATE[0], '') == t and t.startswith(part)
            # the insertion moves the last column over the edge the length sits on
            if L in (C, 2 * C, W, 2 * W):
                assert (L - 1) // W != L // W or E.cols_of(L - (L - 1) // W * W, K) != E.cols_of(L + 1 - (L - 1) // W * W, K)
            sh = shape(c)
            if mode == 1:                            # global: every walk ends in its sequence's last column
                assert [e[1] for e in sh['end'][1:]] == [L, L + 1, 2 * L // 3]
            assert len(sh['indeg']) >= L + 1
    assert 2 * W + 1 - 2 * W == 1                  # a last pass of one column


def test_source_distance_the_far_edge_is_exactly_as_many_ranks_long_as_named():
    cases = cases_of('source distance')
    named = set()
    for c in cases:
        sh = shape(c)
        cp, dist = c.what['cp'], c.what['dist']
        assert E.cols_of(len(c.seqs[0]), K) == cp == E.cols_of(max(len(s) for s in c.seqs), K) and len(c.seqs) == 4
        assert int(sh['dist'].max()) == dist, (c.what, c.algorithm, int(sh['dist'].max()))
        # (a substitution's aligned pair puts two ranks between its neighbours as well: distance 2 is not the planted edge's alone)
        assert int((sh['dist'] == dist).sum()) == 1 or dist == 2
        far = [r for r in range(len(sh['dist'])) if sh['dist'][r] == dist and sh['indeg'][r] == 2 and sh['aligned'][r] == 1][0]
        assert sh['indeg'][far] == 2
        if c.what['form'] == 'deletion':
            # two sequences took the far edge: the second made it with a vertical run, the third read the far source on a diagonal step
            assert (sh['weight'][far] == 4 or dist == 2) and list(sh['vrun']) == [0, dist - 1, 0, 0]
        else:
            assert list(sh['hrun'][1:]) == [dist - 1, 0, 0] or c.algorithm == 0                   # the template edge spans the chain
            assert sh['weight'][far] >= 4
        named.add((c.algorithm, cp, dist, c.what['form']))
    for mode in (0, 1, 2):
        for form in ('deletion', 'insertion'):
            for cp in range(1, K['POA_MAXCP'] + 1):
                ring = K['RING'][cp]
                assert {(mode, cp, d, form) for d in (2, ring - 1, ring, ring + 1)} <= named
            assert (mode, K['POA_MAXCP'], 2 * K['POA_BAND'] + 9, form) in named
    assert 2 * K['POA_BAND'] + 9 - 1 >= 2 * K['POA_BAND'] + 8


def _check_in_edge_case(c):
    d = c.what['indeg']
    sh = shape(c)
    assert int(sh['indeg'].max()) == d and int((sh['indeg'] == d).sum()) == 1, (d, c.algorithm, int(sh['indeg'].max()))
    return sh, int(np.argmax(sh['indeg']))


def test_in_edges_one_node_has_exactly_the_named_in_degree_and_the_consensus_runs_through_the_last_edge():
    cases = cases_of('in-edges')
    P, A = K['POA_MAXP'], K['POA_MAXP_ALL']
    for mode in (0, 1, 2):
        assert {c.what['indeg'] for c in cases if c.algorithm == mode} == {3, 4, P, P + 1, 14, 15, 16, A - 1, A}
    for c in cases:
        d = c.what['indeg']
        sh, node = _check_in_edge_case(c)
        R = E.in_edge_repeats(d)
        assert R >= 3 and len(c.seqs) == d + R - 1 and c.seqs[-1] == c.seqs[-2] == c.seqs[d - 1] and c.seqs[d - 2] != c.seqs[d - 1]
        assert len(c.seqs[0]) - len(c.seqs[-1]) == d - 1 and len(c.seqs[-1]) == 2 * E.FLANK
        # the last predecessor added is the heaviest in-edge of the node: created by sequence d, raised by the two behind it
        assert sh['weight'][node] == 2 * R and sorted(sh['indeg'])[-2] == 1
        cons, msa, scores = want_of(c)
        assert cons == c.seqs[-1] and scores[-1] == 10 * len(c.seqs[-1])
        # every row is its sequence padded inside the motif: one new predecessor per sequence
        for k, row in enumerate(msa[:d]):
            assert row == c.seqs[0][:len(c.seqs[0]) - E.FLANK - k] + '-' * k + c.seqs[0][-E.FLANK:], (d, c.algorithm, k)
    ref = E.in_edges_refused(K)
    sh = shape(ref)
    assert int(sh['indeg'].max()) == A + 1 == ref.what['indeg'] and want_of(ref)[0] is not None


def test_overflow_table_the_totals_are_exact_and_the_entries_of_different_nodes_alternate():
    P, A, CAP = K['POA_MAXP'], K['POA_MAXP_ALL'], K['POA_OVF_CAP']
    for c in cases_of('overflow table'):
        sh = shape(c)
        deg = c.what['degrees']
        assert len(deg) == E.OVERFLOW_JUNCTIONS and len(set(deg)) > 1 and min(deg) > P and max(deg) == A
        assert sorted(int(x) for x in sh['indeg'] if x > 1) == sorted(deg)
        assert sum(max(0, int(x) - P) for x in sh['indeg']) == E.overflow_total(deg, K) > 0
        # sequence k (k >= POA_MAXP) adds an in-edge at every junction of in-degree above k: several nodes per sequence
        assert sum(1 for d in deg if d > P + 1) >= 10
    assert E.overflow_total(E.overflow_capacity_degrees(K), K) == CAP and E.overflow_total(E.overflow_capacity_degrees(K, 1), K) == CAP + 1


@pytest.mark.parametrize('extra', [0, 1])
def test_overflow_capacity_pair_totals_the_table_and_one_entry_more(extra):
    """(the device runs the case at capacity only: the pair took it 46 s, see tests/test_gpu_poa_edges.py; that one entry more is one
    entry more is still proved here)"""
    P, CAP = K['POA_MAXP'], K['POA_OVF_CAP']
    c = E.overflow_capacity(K, extra)
    sh = shape(c)
    assert sorted(int(x) for x in sh['indeg'] if x > 1) == sorted(c.what['degrees'])
    assert sum(max(0, int(x) - P) for x in sh['indeg']) == CAP + extra == c.what['total']
    assert max(len(s) for s in c.seqs) > K['POA_MAX_COPY']           # the wide form of the pass


def test_weights_sit_on_both_sides_of_255_and_the_bundle_has_a_choice():
    cases = cases_of('weights')
    assert {c.what['weight'] for c in cases} == {254, 256, 258}
    for c in cases:
        n = c.what['weight'] // 2
        sh = shape(c)
        assert len(c.seqs) == n + 3 and c.seqs.count(c.seqs[0]) == n and len(c.seqs[0]) == 30
        assert c.min_coverage in (0, (len(c.seqs) + 1) // 2)
        assert sorted(set(int(x) for x in sh['weight'])) == [0, 6, 2 * n, 2 * n + 6]
        assert int((sh['indeg'] == 2).sum()) == 1 and int((sh['aligned'] == 2).sum()) == 6          # the minority branch: three aligned pairs, one node where it joins
        assert want_of(c)[0] == c.seqs[0]
    assert {(c.min_coverage > 0, c.what['weight']) for c in cases} == {(a, w) for a in (False, True) for w in (254, 256, 258)}
    counts = cases_of('score counts')
    assert [len(c.seqs) for c in counts] == [64, 65, 66] == [c.what['count'] for c in counts]
    for c in counts:
        assert len(want_of(c)[2]) == len(c.seqs) and want_of(c)[2][1] != want_of(c)[2][2]


def test_graph_size_the_node_counts_and_lengths_are_exact():
    cases = cases_of('graph size')
    S, R, M = K['POA_SORT_LDS'], K['POA_LDS_SCORES'], K['POA_MAX_COPY']
    for mode, scores in E.SIZE_MODES:
        mine = [c for c in cases if (c.algorithm, c.scores) == (mode, scores)]
        assert [c.what['nodes'] for c in mine if 'nodes' in c.what] == [S - 1, S, S + 1, R - 1, R, R + 1]
        assert [c.what['length'] for c in mine if 'length' in c.what] == [M - 1, M, M + 1]
        for c in mine:
            sh = shape(c)
            if 'nodes' in c.what:
                assert len(sh['indeg']) == c.what['nodes'] and len(c.seqs) == 2 and len(c.seqs[0]) < c.what['nodes'], c.what
            else:
                assert max(len(s) for s in c.seqs) == len(c.seqs[0]) == c.what['length'] and int(sh['vrun'].max()) == 1


def test_ties_both_cells_score_the_same_and_the_oracle_takes_the_smaller_row_then_column():
    kinds = set()
    for c, proof in E.tie_cases(K):
        sh = shape(c)
        other = shape_of(proof, c.algorithm, c.scores)
        score = want_of(c)[2][1]
        assert score == oracle_lib.oracle_poa(proof, c.algorithm, True, *c.scores, with_scores=True)[2][1] > 0
        what = c.what
        m = len(c.seqs[1])
        if what['tie'] == 'rows':
            assert sh['end'][1][1] == other['end'][1][1] == what['column'] and sh['end'][1][0] == len(E.ROW_TIE_U) < other['end'][1][0] == len(c.seqs[0])
        else:
            first, second = what['columns']
            assert sh['end'][1] == (other['end'][1][0], first) and other['end'][1][1] == second and second <= m
            if what['tie'] in ('halves', 'neighbours', 'lanes'):
                cp = what['cp']
                assert E.cols_of(m, K) == cp and m <= 128 * cp
                la, lb = (first - 1) // (2 * cp), (second - 1) // (2 * cp)
                ra, rb = (first - 1) % (2 * cp), (second - 1) % (2 * cp)
                if what['tie'] == 'halves':          # one lane, one register: its low and its high half
                    assert la == lb and ra < cp and rb == ra + cp
                elif what['tie'] == 'neighbours':    # the high half of a lane and the low half of the next
                    assert lb == la + 1 and ra >= cp and rb == ra - cp
                else:
                    assert lb > la + 1
                kinds.add((what['tie'], cp, ra))
            else:
                assert (first - 1) // K['W'] < (second - 1) // K['W']
        # the MSA tells the two apart: the letters of U stand in the graph's column under the first copy only
        kinds.add(what['tie'])
    assert kinds >= {'halves', 'neighbours', 'lanes', 'passes', 'rows'}
    for cp in range(1, K['POA_MAXCP'] + 1):
        assert {(t, cp, r) for t, r in [('halves', r) for r in range(cp)] + [('neighbours', r) for r in range(cp, 2 * cp)]} <= kinds
    passes = [c.what['columns'] for c, _ in E.tie_cases(K) if c.what['tie'] == 'passes']
    assert (K['W'], K['W'] + 1) in passes and any((b - 1) // K['W'] - (a - 1) // K['W'] == 2 for a, b in passes)


def test_walks_the_runs_are_exactly_as_long_as_named():
    cases = cases_of('walks')
    h = K['BT_RING'] // 2
    want_h = {K['BT_DRIFT'] - 1, K['BT_DRIFT'], K['BT_W'], 64, h - 1, h, h + 1, K['BT_RING'], K['BT_RING'] + 1}
    for mode in (0, 1, 2):
        assert {c.what['hrun'] for c in cases if c.algorithm == mode and 'hrun' in c.what} == want_h
        assert {c.what['vrun'] for c in cases if c.algorithm == mode and 'vrun' in c.what} == {47, 48, 49, 64, 65}
    for c in cases:
        sh = shape(c)
        if 'hrun' in c.what:
            assert list(sh['hrun']) == [0, c.what['hrun'], 0] and list(sh['vrun']) == [0, 0, 0], (c.what, c.algorithm)
            # flanks of 40; where the end of the sequence is free (local, overlap) a flank must outweigh the gap to stay in the alignment
            flank = E.walk_flank(c.what['hrun'], c.algorithm)
            assert len(c.seqs[1]) == 2 * flank + c.what['hrun'] and flank >= E.WALK_FLANK and (flank == E.WALK_FLANK or c.algorithm != 1)
            assert c.algorithm == 1 or c.scores[0] * flank > E.gap_cost(c.what['hrun'])
        else:
            assert list(sh['vrun']) == [0, c.what['vrun'], 0] and list(sh['hrun']) == [0, 0, 0], (c.what, c.algorithm)
        if c.algorithm == 0:
            assert want_of(c)[2][1] > 10 * E.WALK_FLANK        # both flanks are inside the local alignment


def test_band_sweep_the_leading_insertions_straddle_the_band_width():
    cases = cases_of('band sweep')
    B = K['POA_BAND']
    for mode, scores in E.BAND_MODES:
        mine = [c for c in cases if c.algorithm == mode]
        assert [c.what['lead'] for c in mine] == list(range(B - 8, B + 9, 2))
        for c in mine:
            k = c.what['lead']
            sh = shape(c)
            assert len(c.seqs) == 4 and len(c.seqs[3]) == 300 + k > 2 * B + 64          # the planes keep a band for this length
            # the walk of the last sequence starts k columns off the graph's diagonal
            assert sh['end'][3][1] == 300 + k and want_of(c)[2][3] >= c.scores[0] * 300 - (0 if mode == 0 else E.gap_cost(k))
            if mode == 1:
                assert sh['hrun'][3] == k


def test_tandem_reads_have_the_named_periods():
    C, W = K['C'], K['W']
    reads = E.tandem_reads(K)
    assert [len(r) // E.TANDEM_COPIES for r in reads] == [C, C + 1, W, W + 1, W + C, W + C + 1]
    for r in reads:
        p = len(r) // E.TANDEM_COPIES
        assert r == r[:p] * E.TANDEM_COPIES and set(r) <= set('ACGT')
        seg, ccs, period = oracle_lib.oracle_find_consensus(r)
        assert seg == ';'.join('%d-%d' % (k * p, (k + 1) * p) for k in range(E.TANDEM_COPIES)) and ccs == r[:p], (p, seg)


# ----------------------------------------------------------------------------------------------------------------------------
# the row formulation (tools/poa_model.py) on the cases it can run
# ----------------------------------------------------------------------------------------------------------------------------
def _cells(case):
    """an upper bound: every sequence against the final graph; a row costs the model about as much as 200 of its cells"""
    return len(shape(case)['indeg']) * sum(len(s) + 200 for s in case.seqs[1:])


def model_cases(name):
    """the cases the model can take (at most Graph.MAXP in-edges in place -- it has no overflow table) within MODEL_CELLS each,
    cheapest first"""
    return [c for c in sorted(cases_of(name), key=_cells)
            if _cells(c) <= MODEL_CELLS and c.what.get('indeg', 0) <= poa_model.Graph.MAXP and 'degrees' not in c.what]


def model_subset(name):
    """... of which the model is held to the oracle on the cheapest within SET_CELLS.  Every case of model_cases runs in well under a
    second, but all of them together take the model a minute and a half, and this file is to stay under a minute beside the oracle's
    share: the budget keeps every set's cheapest shapes (all register counts of the source distances, all ties, all walks but the
    longest, in-degrees up to POA_MAXP), and the planted faults below are hunted through all of model_cases, cheapest first."""
    out, total = [], 0
    for c in model_cases(name):
        if total + _cells(c) <= SET_CELLS:
            out.append(c); total += _cells(c)
    return out


def _letters(s):
    return np.frombuffer(s.encode('latin-1'), dtype=np.uint8).astype(np.int64)


def _text(a):
    return bytes(int(x) for x in a).decode('latin-1')


def _model(case, model=poa_model):
    cons, rows, scores, _order = model.poa([_letters(s) for s in case.seqs], case.algorithm, True, *case.scores, min_coverage=case.min_coverage)
    return _text(cons), [_text(r) for r in rows], scores


MODEL_SETS = [n for n in E.SETS if n not in ('overflow table', 'graph size')]


@pytest.mark.parametrize('name', MODEL_SETS)
def test_model_equals_the_oracle_on_the_cases_it_can_run(name):
    sub = model_subset(name)
    assert sub, name
    for c in sub:
        assert _model(c) == tuple(want_of(c)), (name, c.what, c.algorithm)


# ----------------------------------------------------------------------------------------------------------------------------
# the sets have teeth
# ----------------------------------------------------------------------------------------------------------------------------
# (name, text of tools/poa_model.py, what replaces it, the sets asked in turn)
MUTANTS = [
    ('a later row wins a tie of the best cell', 'if H[jm] > best:', 'if H[jm] >= best:', ('ties',)),
    ('the last column wins a tie within a row', 'jm = int(np.argmax(H[1:])) + 1', 'jm = L - int(np.argmax(H[1:][::-1]))', ('ties',)),
    ('the third source of a row is dropped', 'H, dF, dO, bits, slots, dE, dQ = dp_row(P, G.code[v], seq, [rows[p] for p in pr], col0)',
     'H, dF, dO, bits, slots, dE, dQ = dp_row(P, G.code[v], seq, [rows[p] for p in pr[:2]], col0)', ('in-edges',)),
    ('edge weights wrap at 8 bits', 'for u, w in zip(G.pred[v], G.pw[v]):', 'for u, w in zip(G.pred[v], [x & 255 for x in G.pw[v]]):', ('weights',)),
    ('the second gap piece of a vertical gap is not handed to the next row', 'dO[1:] = np.maximum(os_new - h1, -1)', 'dO[1:] = -1', ('walks',)),
    ('the horizontal gap states are not handed to the next pass', 'run = np.maximum.accumulate(m0 - k * ext)',
     'run = np.concatenate([np.maximum.accumulate(x) for x in np.split(m0 - k * ext, range(%d, L + 1, %d))])' % (K['W'], K['W']), ('walks',)),
    ('a far source row is read one row off', 'pr = [G.rank[u] for u in G.pred[v]] or [0]',
     'pr = [G.rank[u] + (r - G.rank[u] >= 4) for u in G.pred[v]] or [0]', ('source distance',)),
]


def _mutant(old, new):
    path = os.path.join(os.path.dirname(os.path.abspath(poa_model.__file__)), 'poa_model.py')
    with open(path) as f:
        src = f.read()
    assert src.count(old) == 1, (old, src.count(old))
    ns = {'__name__': 'poa_model_mutant'}
    exec(compile(src.replace(old, new), path, 'exec'), ns)

    class _M(object):
        poa = staticmethod(ns['poa'])
    return _M


def _disagrees(model, case):
    try:
        return _model(case, model=model) != tuple(want_of(case))
    except (AssertionError, IndexError, ValueError, OverflowError):        # a walk that leaves the matrix is a disagreement too
        return True


@pytest.mark.parametrize('name,old,new,sets', MUTANTS, ids=[m[0] for m in MUTANTS])
def test_a_planted_fault_in_the_model_is_caught_by_a_named_set(name, old, new, sets):
    model = _mutant(old, new)
    caught = [s for s in sets if any(_disagrees(model, c) for c in model_cases(s))]
    print('%s: caught by %s' % (name, ', '.join(caught)))
    assert caught == list(sets), (name, caught)


def test_the_unchanged_source_passes_where_the_mutants_fail():
    model = _mutant('def poa(', 'def poa(')
    for s in ('ties', 'in-edges'):
        assert not any(_disagrees(model, c) for c in model_subset(s)[:6])
