"""K2 (the repeat scan of csrc/ccs_poa.hip) through Context.ccs_batch on the edge sets of tests/ccs_edges.py: launch classes, thresholds,
periods at their limits, plateaus across lanes and waves, harmonics, the cap of cuts, ties of the vote and of the anchor's keys, N and
odd codes, long chains.  For every read the status is 0, period, nseg and the segments equal clo_ccs_segments plus the tail rule -- K2
read on its own, not through K3's answer -- and (segments, ccs) equals oracle_find_consensus.  That each case reaches its edge is proved
on the CPU from the oracle's trace (tests/test_ccs_edges_host.py).

Reads of at most 1024 bases go three ways, whose rows must be equal: in a batch whose longest read has at most 960 bases (the one-wave
kernel at its natural class), in a batch padded with a read of 1024 bases (four waves), and in that batch under CLH_K2_ONE_WAVE (the
one-wave kernel at the LDS layout of the larger class).  Longer reads run as four waves and under CLH_K2_ONE_WAVE."""
import numpy as np
import pytest

import ccs_edges as E
import oracle_lib

pytestmark = pytest.mark.gpu

K = E.constants()
WIDE = K['K2_WIDE_FROM']


def ccs_batch(reads):
    from ciri_long_amd import hip
    data, off = hip.pack(reads)
    rows, segs, ccs = hip.default_context().ccs_batch(data, off)
    return rows, segs, ccs, off


def check(reads, got, label):
    """every read of a batch against the oracle: K2's own answer first, then the consensus"""
    rows, segs, ccs, off = got
    assert len(rows) == len(reads)
    for k, r in enumerate(reads):
        want = E.want_of(r, K)
        where = (label, k, len(r))
        assert int(rows[k]['status']) == 0, where
        n = int(rows[k]['nseg'])
        assert int(rows[k]['period']) == want['period'], where
        assert n == len(want['segs']) and [tuple(int(x) for x in s) for s in segs[k, :n]] == want['segs'], where
        if n:
            seg = ';'.join('%d-%d' % (segs[k, i, 0], segs[k, i, 1]) for i in range(n))
            cons = (seg, oracle_lib.decode(ccs[off[k]:off[k] + int(rows[k]['ccs_len'])]))
        else:
            cons = (None, None)
        assert cons == want['consensus'], where


def same_rows(a, ia, b, ib, label):
    for x, y in zip(ia, ib):
        assert a[0][x] == b[0][y] and (a[1][x] == b[1][y]).all(), (label, x, y)


def three_ways(name, monkeypatch):
    cases = E.SETS[name](K)
    reads = [c.read for c in cases]
    assert reads and max(len(r) for r in reads) > 0
    narrow = [k for k, r in enumerate(reads) if len(r) <= WIDE - 64]
    padded = reads + [E.filler(K, WIDE)]
    if narrow:
        one = ccs_batch([reads[k] for k in narrow])               # one wave, its natural class
        check([reads[k] for k in narrow], one, (name, 'one wave'))
    x4 = ccs_batch(padded)                                        # four waves
    check(padded, x4, (name, 'x4'))
    monkeypatch.setenv('CLH_K2_ONE_WAVE', '1')                    # read by the launcher at every launch
    forced = ccs_batch(padded)
    monkeypatch.delenv('CLH_K2_ONE_WAVE')
    check(padded, forced, (name, 'one wave forced'))
    same_rows(x4, range(len(padded)), forced, range(len(padded)), name)
    if narrow:
        same_rows(one, range(len(narrow)), x4, narrow, name)


SHORT_SETS = [n for n in E.SETS if n not in ('classes',)]


@pytest.mark.parametrize('name', SHORT_SETS)
def test_set_by_one_wave_by_four_and_by_one_wave_forced(name, monkeypatch):
    three_ways(name, monkeypatch)


def test_every_class_length_alone(monkeypatch):
    """960 .. 16001 bases, each alone in its batch: its own class, bucket count and kernel; then the same under CLH_K2_ONE_WAVE"""
    reads = [c.read for c in E.classes(K)]
    alone = [ccs_batch([r]) for r in reads]
    for r, got in zip(reads, alone):
        check([r], got, ('classes alone', len(r)))
    monkeypatch.setenv('CLH_K2_ONE_WAVE', '1')
    for r, got in zip(reads, alone):
        forced = ccs_batch([r])
        check([r], forced, ('classes alone, one wave forced', len(r)))
        same_rows(got, [0], forced, [0], len(r))


def test_all_class_lengths_in_one_shuffled_batch(monkeypatch):
    """every class in one plan: the classes' k2_begin, and two long reads of different length in the long kernel's slots"""
    cases = E.classes(K)
    reads = [cases[k].read for k in E.mixed_order(len(cases))]
    assert sum(len(r) > K['kK2LdsMax'] for r in reads) == 2
    mixed = ccs_batch(reads)
    check(reads, mixed, 'classes mixed')
    monkeypatch.setenv('CLH_K2_ONE_WAVE', '1')
    forced = ccs_batch(reads)
    check(reads, forced, 'classes mixed, one wave forced')
    same_rows(mixed, range(len(reads)), forced, range(len(reads)), 'classes mixed')


def test_a_plan_run_twice_starts_from_clean_records():
    """one ccs_plan, two runs: the second on reads of the same lengths of which every other one holds no repeat"""
    import torch
    from ciri_long_amd import hip
    first = [c.read for c in E.plateaus(K)] + [c.read for c in E.cuts(K)]
    rng = E._rng('second run')
    second = [r if k % 2 else E.dna(rng, len(r)) for k, r in enumerate(first)]
    assert any(E.want_of(r, K)['period'] == 0 for r in second)
    data, off = hip.pack(first)
    plan = hip.default_context().ccs_plan(off)
    for reads in (first, second, first):
        data, _ = hip.pack(reads)
        d = torch.from_numpy(data.view(np.uint8)).cuda()
        plan.run(d.data_ptr(), torch.cuda.current_stream().cuda_stream)
        rows, segs, ccs = plan.fetch()
        check(reads, (rows, segs, ccs, off), 'plan run again')
    plan.close()
