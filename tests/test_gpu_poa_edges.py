"""K3 (partial-order consensus, csrc/ccs_poa.hip) through poa_batch on the edge sets of tests/poa_edges.py: pass widths, source
distances, in-edges and the overflow table, weights around 255, graph sizes, ties of the best cell, walks across the back-track's
staging.  Every case must equal oracle/poa_oracle.c in consensus, every MSA row and every end-cell score; that each case reaches its
edge is proved on the CPU from the oracle's shape record (tests/test_poa_edges_host.py).  The cases of a set that share mode and scores
go to the device as the groups of ONE call, between two ordinary groups, so edge graphs and plain ones share a launch."""
import numpy as np
import pytest

import oracle_lib
import poa_edges as E

pytestmark = pytest.mark.gpu

K = E.constants()
_want = {}


def want_of(seqs, algorithm, scores, min_coverage):
    """the oracle's (consensus, msa rows, scores), computed once and shared"""
    key = (tuple(seqs), algorithm, scores, min_coverage)
    if key not in _want:
        _want[key] = oracle_lib.oracle_poa(seqs, algorithm, True, *scores, with_scores=True, min_coverage=min_coverage)
    return _want[key]


def ordinary_group():
    """a family of five with the usual errors, no edge in it"""
    rng = E._rng('ordinary')
    t = E.dna(rng, 150)
    return [t, E.substitute(t, [30, 90]), t[:60] + t[63:], t[:100] + 'GA' + t[100:], t[20:]]


def poa_groups(groups, algorithm, scores, min_coverage=0):
    from ciri_long_amd import hip
    flat = [s for g in groups for s in g]
    data, off = hip.pack_raw(flat)
    goff = np.cumsum([0] + [len(g) for g in groups]).astype(np.int64)
    return hip.default_context().poa_batch(data, off, goff, algorithm=algorithm, scores=scores, min_coverage=min_coverage, genmsa=True,
                                           with_scores=True, raw=True)


def check_batches(cases):
    """every case, in one call per (mode, scores, min_coverage), against the oracle; nothing dropped"""
    from ciri_long_amd import hip
    assert cases
    for (algorithm, scores, mc), batch in E.batches(cases):
        groups = [ordinary_group()] + [c.seqs for c in batch] + [ordinary_group()]
        got = poa_groups(groups, algorithm, scores, mc)
        stats = hip.default_context().poa_last_stats()
        assert len(got) == len(groups)
        for k, (g, seqs) in enumerate(zip(got, groups)):
            what = batch[k - 1].what if 0 < k <= len(batch) else 'ordinary'
            want = want_of(seqs, algorithm, scores, mc)
            assert g[2] == want[2][:65], (what, algorithm, scores, 'scores')
            assert g[0] == want[0], (what, algorithm, scores, 'consensus')
            assert g[1] == want[1], (what, algorithm, scores, 'msa')
        assert stats['dropped'] == {}, stats


def _of_mode(name, mode, scores=None):
    return [c for c in E.SETS[name](K) if c.algorithm == mode and (scores is None or c.scores == scores)]


@pytest.mark.parametrize('mode,scores', E.PASS_MODES, ids=['local', 'local-not-simple', 'global', 'overlap', 'global-convex'])
def test_pass_widths(mode, scores):
    """sequences of C-1 .. 2W+1 letters (C = 128, W = 128 POA_MAXCP): one, two, .. POA_MAXCP registers per lane, full passes, a last
    pass of one column, a substitution in the first and last column of every pass"""
    check_batches(_of_mode('pass widths', mode, scores))


@pytest.mark.parametrize('mode', [0, 1, 2])
def test_source_distance(mode):
    """a source row 2, RING-1, RING, RING+1 ranks back for every register count, and one outside the target row's band: read from the LDS
    ring or from the planes by the sequence that comes after the edge exists"""
    check_batches(_of_mode('source distance', mode))


@pytest.mark.parametrize('mode', [0, 1, 2])
def test_in_edges(mode):
    """one node with 3, 4, POA_MAXP, POA_MAXP+1, 14, 15, 16, POA_MAXP_ALL-1, POA_MAXP_ALL in-edges, the last of them raised in weight until
    the consensus runs through it"""
    check_batches(_of_mode('in-edges', mode))


def test_in_edges_one_more_than_the_kernel_keeps_is_refused_and_the_context_answers_on():
    from ciri_long_amd import hip
    c = E.in_edges_refused(K)
    assert want_of(c.seqs, c.algorithm, c.scores, 0)[0] is not None          # the oracle answers it
    with pytest.raises(hip.ClhError, match='status 2'):
        poa_groups([c.seqs], c.algorithm, c.scores)
    assert hip.default_context().poa_last_stats()['dropped'] == {2: 1}
    check_batches([E.Case(ordinary_group(), c.algorithm, c.scores, 0, 'after a refusal')])


@pytest.mark.parametrize('mode', [0, 1, 2])
def test_overflow_table_entries_of_several_nodes_interleave(mode):
    """12 junctions past POA_MAXP in one graph: every sequence adds an entry for each of them"""
    check_batches(_of_mode('overflow table', mode))


def test_overflow_table_at_capacity():
    """junctions whose overflow entries total exactly POA_OVF_CAP, in sequences of about 3400 letters (the wide form of the pass), global
    mode only.  Measured on an MI355X: 23.7 s for this case and 22.5 s for the same with one entry more, which is refused with status 2
    -- more than 15 s together, so only the case at capacity is kept.  (Flanks of two letters, which keep the pair within POA_MAX_COPY
    and in the packed form, took 22.8 s and 21.7 s: the time goes with the graph's 2048 overflow entries, not with the form of the
    pass.)  A refusal past a limit of the table's kind is still held: POA_MAXP_ALL + 1 in-edges, above."""
    import time
    full = E.overflow_capacity(K)
    want_of(full.seqs, full.algorithm, full.scores, 0)
    t0 = time.perf_counter()
    check_batches([full])
    print('overflow table at capacity: %.1f s' % (time.perf_counter() - t0))


def test_weights_on_both_sides_of_255():
    """127, 128, 129 identical sequences and a minority branch: in-edge weights 254, 256, 258, with and without min_coverage"""
    check_batches(E.weights(K))


def test_scores_of_the_first_65_sequences():
    """64, 65, 66 sequences with_scores: the 65th score is right and there is no 66th"""
    cases = E.score_counts(K)
    check_batches(cases)
    for c in cases:
        got = poa_groups([c.seqs], c.algorithm, c.scores)[0]
        want = want_of(c.seqs, c.algorithm, c.scores, 0)
        assert len(got[2]) == min(65, len(c.seqs)) and got[2] == want[2][:65] and got[2][-1] == want[2][min(65, len(c.seqs)) - 1]


@pytest.mark.parametrize('mode', [0, 1])
def test_graph_size(mode):
    """graphs of exactly POA_SORT_LDS-1 .. +1 nodes (the sort leaves LDS) and POA_LDS_SCORES-1 .. +1 (the consensus scores do);
    sequences of POA_MAX_COPY-1 .. +1 letters (the last runs the wide form)"""
    check_batches(_of_mode('graph size', mode))


def test_ties_of_the_best_cell():
    """local mode, the same score in one row at two columns -- in the two halves of a register, in neighbouring lanes, in far lanes, in two
    passes -- and in one column at two rows: spoa takes the smallest row, then the smallest column, and the MSA shows which one was taken"""
    check_batches(E.ties(K))


@pytest.mark.parametrize('mode', [0, 1, 2])
def test_walks(mode):
    """horizontal runs of BT_DRIFT-1 .. BT_RING+1 columns (the staged band's drift and width, the result ring and its flush) and vertical
    runs of 47 .. 65 rows (the re-stage after 48)"""
    check_batches(_of_mode('walks', mode))


def test_band_sweep_straddles_the_fallback():
    """a leading insertion of POA_BAND-8 .. POA_BAND+8 letters in front of a 300-letter template: every step equals the oracle; summed over
    the modes, no walk leaves the band of stored cells at the first step and some do at the last"""
    from ciri_long_amd import hip
    misses = {}
    for c in E.band_sweep(K):
        check_batches([c])          # (its own call: the ordinary groups beside it stay inside the band)
        misses[c.what['lead']] = misses.get(c.what['lead'], 0) + hip.default_context().poa_last_stats()['band_misses']
    steps = E.band_steps(K)
    print('band misses by leading insertion:', [(k, misses[k]) for k in steps])
    assert misses[steps[0]] == 0 and misses[steps[-1]] > 0, misses


def test_exact_tandem_reads_enter_k3_from_k2_at_the_pass_edges():
    """find_consensus on 8 exact copies of a unit of C, C+1, W, W+1, W+C, W+C+1 letters"""
    from ciri_long_amd import pyccs
    reads = E.tandem_reads(K)
    got = pyccs.find_consensus_batch(reads)
    for k, r in enumerate(reads):
        want = oracle_lib.oracle_find_consensus(r)
        assert want[0] is not None and got[k] == want[:2], (len(r) // E.TANDEM_COPIES, got[k][0], want[0])
