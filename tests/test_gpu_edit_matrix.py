"""Edit-distance matrices of whole groups built on the device (csrc/edit_matrix.hip in front of K4): hip.Context.edit_matrix_batch,
hip.EditMatrixPlan, utils.pairwise_distance_groups, utils.compress_seq_batch and the collapse route over them.  The checker is
oracle_lib.oracle_edit_distance on utils.compress_seq outputs; the pair route (utils.distance_batch) is compared as well."""
import ctypes as C
import random

import numpy as np
import pytest

import oracle_lib

pytestmark = pytest.mark.gpu


def _ctx():
    from ciri_long_amd import hip
    return hip.default_context()


def _hpc(s):
    """utils.compress_seq, for bytes as well"""
    from ciri_long_amd import utils
    return utils.compress_seq(s) if isinstance(s, str) else utils.compress_seq(s.decode('latin-1')).encode('latin-1')


def _mutated(rng, s, rate, alpha='ACGT'):
    out = []
    for c in s:
        r = rng.random()
        if r < rate / 3:
            out.append(rng.choice(alpha))
        elif r < 2 * rate / 3:
            continue
        elif r < rate:
            out += [c, rng.choice(alpha)]
        else:
            out.append(c)
    return ''.join(out)


def _check_group(seqs, dist, lens, compressed, every=1):
    """one group of a fetch against the oracle (every `every`-th pair) and the pair route (all pairs)"""
    from ciri_long_amd import utils
    ref = [_hpc(s) for s in seqs] if compressed else list(seqs)
    n = len(seqs)
    ii, jj = np.triu_indices(n, 1)
    assert dist.dtype == np.int32 and lens.dtype == np.int32
    assert len(dist) == n * (n - 1) // 2 and lens.tolist() == [len(r) for r in ref]
    if n < 2:
        return
    pairs = utils.distance_batch([ref[i] for i in ii], [ref[j] for j in jj])
    assert np.array_equal(dist, pairs)
    for q in range(0, len(ii), every):
        assert int(dist[q]) == oracle_lib.oracle_edit_distance(ref[ii[q]], ref[jj[q]]), (n, int(ii[q]), int(jj[q]))


def test_group_sizes_offsets_and_condensed_order():
    rng = random.Random(101)
    groups = []
    for n in (0, 1, 2, 0, 3, 50, 51, 0):
        base = ''.join(rng.choice('ACGT') for _ in range(rng.randint(20, 200)))
        groups.append([_mutated(rng, base, 0.15) if rng.random() < 0.8 else ''.join(rng.choice('ACGT') for _ in range(rng.randint(1, 200)))
                       for _ in range(n)])
    res = _ctx().edit_matrix_batch(groups)
    assert len(res) == len(groups)
    for g, r in zip(groups, res):
        assert len(r) == 2
        _check_group(g, r[0], r[1], False)
    assert all(len(res[k][0]) == 0 and len(res[k][1]) == 0 for k in (0, 3, 7))
    assert len(res[1][0]) == 0 and len(res[1][1]) == 1
    assert _ctx().edit_matrix_batch([]) == []


def test_one_group_of_2000_strings_every_pair():
    """1 999 000 pairs: where a pair-index inversion that is not exact puts a distance in the wrong place"""
    from ciri_long_amd import utils
    rng = random.Random(7)
    seqs = [''.join(rng.choice('ACGT') for _ in range(rng.randint(5, 12))) for _ in range(2000)]
    (dist, lens), = _ctx().edit_matrix_batch([seqs])
    ii, jj = np.triu_indices(2000, 1)
    assert len(dist) == 1999000 and lens.tolist() == [len(s) for s in seqs]
    assert np.array_equal(dist, utils.distance_batch([seqs[i] for i in ii], [seqs[j] for j in jj]))
    for q in list(range(0, 1999000, 4001)) + [1998999]:
        assert int(dist[q]) == oracle_lib.oracle_edit_distance(seqs[ii[q]], seqs[jj[q]])


def _cyc(letters, n, at=0):
    return ''.join(letters[(at + k) % len(letters)] for k in range(n))


def test_compression_edges_strings_and_lengths():
    from ciri_long_amd import utils
    crossing = (_cyc('ACGT', 62) + 'T' * 4 + _cyc('ACG', 60) + 'A' * 5 + _cyc('CGTA', 123) + 'G' * 6 + _cyc('TCA', 10))
    assert crossing[62:66] == 'TTTT' and crossing[126:131] == 'AAAAA' and crossing[254:260] == 'GGGGGG'
    seqs = [b'', b'A', b'A' * 300, crossing.encode(), b'C' * 63 + b'GG' + b'C' * 63 + b'GG', b'ACGTTTT', b'ACGA', b'AAGT', b'\xff' * 70, b'\x00' * 70, b'',
            b'\x00\x00\xff\xff\x00', b'T' * 64, b'T' * 65 + b'A']
    (dist, lens, strs), = _ctx().edit_matrix_batch([seqs], hpc=True)
    assert strs == [_hpc(s) for s in seqs]
    assert strs[2] == b'A' and strs[6] == b'ACGA' and strs[7] == b'AGT' and strs[8] == b'\xff' and strs[9] == b'\x00'
    _check_group(seqs, dist, lens, True)
    # the compression alone, str in -> str out
    texts = [s.decode('latin-1') for s in seqs[:8]]
    assert utils.compress_seq_batch(texts) == [utils.compress_seq(t) for t in texts]
    assert utils.compress_seq_batch([]) == []


def test_class_edges_after_compression():
    """pattern lengths at the lane-group borders AFTER compression, from strings whose raw lengths sit in a higher class: x is run-free with
    the edge length, inflated into the next class; y is longer raw and shorter compressed; z shorter raw and longer compressed"""
    def inflate(s, raw):
        extra, n = raw - len(s), len(s)
        return ''.join(c * (1 + extra // n + (1 if k < extra % n else 0)) for k, c in enumerate(s))

    groups = []
    for e in (63, 64, 65, 128, 129, 2048, 2049, 4096, 4097):
        raw = next((t for t in (64, 128, 256, 512, 1024, 2048, 4096) if t >= e), e) + 6
        x = inflate(_cyc('ACGT', e), raw)
        y = inflate(_cyc('ACTG', e - 1, 1), raw + 5)
        z = _cyc('AGCT', e + 3, 2)
        assert len(x) > len(z) and len(_hpc(x)) == e and len(_hpc(y)) == e - 1 and len(y) > len(x) and len(_hpc(z)) == e + 3
        groups.append([x, y, z])
    groups.append([_cyc('ACGT', 4200), _cyc('ACTG', 4200, 3)])                  # both above 4096: the between-pass carry buffers
    rng = random.Random(4)
    long_a = inflate(_cyc('ACG', 3000), 5000)
    groups.append([long_a, inflate(_mutated(rng, _cyc('ACG', 3000), 0.05), 5000)])
    res = _ctx().edit_matrix_batch(groups, hpc=True)
    for g, (dist, lens, strs) in zip(groups, res):
        assert strs == [_hpc(s) for s in g]
        _check_group(g, dist, lens, True)
    assert res[-1][1][0] == 3000 and res[-2][1].tolist() == [4200, 4200]


@pytest.mark.parametrize('alpha', ['ACGT', 'ACDEFGHIKLMN'])
def test_alphabet_planes(alpha):
    rng = random.Random(len(alpha))
    base = ''.join(rng.choice(alpha) for _ in range(150))
    seqs = [base, base, '', _mutated(rng, base, 0.2, alpha), ''.join(rng.choice(alpha) for _ in range(90)), alpha, '', alpha[::-1] * 30]
    assert len(set(''.join(seqs))) == len(alpha)
    for hpc in (False, True):
        res, = _ctx().edit_matrix_batch([seqs], hpc=hpc)
        _check_group(seqs, res[0], res[1], hpc)
        ii, jj = np.triu_indices(len(seqs), 1)
        d = {(i, j): int(v) for i, j, v in zip(ii, jj, res[0])}
        assert d[(0, 1)] == 0 and d[(2, 6)] == 0
        assert d[(0, 2)] == res[1][0] and d[(2, 5)] == len(alpha) and d[(1, 6)] == res[1][1]


def test_plan_reuse_and_timing():
    rng = random.Random(12)
    groups = [[''.join(rng.choice('ACGT') * rng.choice((1, 1, 2, 4)) for _ in range(rng.randint(1, 300))) for _ in range(n)] for n in (30, 1, 17)]
    plan = _ctx().edit_matrix_plan(groups, hpc=True)
    try:
        plan.run()
        first = plan.fetch()
        t1 = plan.timing()
        plan.run()
        second = plan.fetch()
        assert t1 > 0 and plan.timing() > 0
        npairs, nbytes = plan.sizes()
        assert npairs == 30 * 29 // 2 + 17 * 16 // 2 and nbytes == sum(len(_hpc(s)) for g in groups for s in g)
    finally:
        plan.close()
    for g, a, b in zip(groups, first, second):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
        _check_group(g, a[0], a[1], True, every=7)


def test_refusals_and_the_no_room_report(monkeypatch):
    from ciri_long_amd import hip
    ctx = _ctx()
    with pytest.raises(hip.ClhError, match='2\\^31 - 1 pairs'):
        ctx.edit_matrix_plan([['A'] * 65537])
    L = hip.lib()
    data = np.frombuffer(b'ACGTACGT', dtype=np.uint8)
    off = np.array([0, 5, 3], dtype=np.int64); goff = np.array([0, 2], dtype=np.int64)
    assert not L.clh_edit_matrix_plan_create(ctx._h, 2, data.ctypes.data, off.ctypes.data, 1, goff.ctypes.data, 0)
    assert 'ascend' in hip.last_error()
    goff[1] = 3
    off[:] = [0, 3, 8]
    assert not L.clh_edit_matrix_plan_create(ctx._h, 2, data.ctypes.data, off.ctypes.data, 1, goff.ctypes.data, 0)
    out = np.zeros(1, dtype=np.int32); lens = np.zeros(2, dtype=np.int32)
    goff[1] = 2
    assert L.clh_edit_matrix_batch(ctx._h, 2, data.ctypes.data, off.ctypes.data, 1, goff.ctypes.data, 0, out.ctypes.data, 0, lens.ctypes.data, None, 0) == -4
    assert L.clh_edit_matrix_batch(ctx._h, 2, data.ctypes.data, off.ctypes.data, 1, goff.ctypes.data, 0, out.ctypes.data, 1, lens.ctypes.data, None, 0) == 0
    assert out[0] == oracle_lib.oracle_edit_distance('ACG', 'TACGT') and lens.tolist() == [3, 5]
    # a pair above 4096 symbols that finds no room between passes is reported, not skipped
    pair = [_cyc('ACGT', 4200), _cyc('ACTG', 4200, 3)]
    monkeypatch.setenv('CLH_EM_CARRY_BYTES', '4096')
    with pytest.raises(hip.ClhError, match='1 pairs .* found no room'):
        ctx.edit_matrix_batch([pair, ['ACGT', 'AGGT']])
    monkeypatch.delenv('CLH_EM_CARRY_BYTES')
    res = ctx.edit_matrix_batch([pair, ['ACGT', 'AGGT']])
    assert int(res[0][0][0]) == oracle_lib.oracle_edit_distance(*pair) and int(res[1][0][0]) == 1


def _jobs():
    rng = random.Random(2024)
    jobs = []
    for k, n in enumerate([1, 2, 49, 50, 51, 120] + [rng.randint(3, 30) for _ in range(14)]):
        tm = ''.join(rng.choice('ACGT') * rng.choice((1, 1, 1, 2, 3)) for _ in range(400))[:rng.randint(150, 400)]
        other = tm[:len(tm) // 2] + ''.join(rng.choice('ACGT') for _ in range(len(tm) // 2))      # a second isoform
        reads = [('r%d_%d' % (k, i), _mutated(rng, other if i % 5 == 4 else tm, 0.04)) for i in range(n)]
        jobs.append(('circ%d' % k, reads))
    return jobs


def test_collapse_route_equals_the_pair_route(monkeypatch):
    from ciri_long_amd import collapse, utils
    jobs = _jobs()
    assert sorted(len(r) for _, r in jobs)[-3:] == [50, 51, 120] and all(150 * 0.8 < len(s) < 400 * 1.2 for _, r in jobs for _, s in r)
    monkeypatch.delenv('CLH_NO_EDIT_MATRIX', raising=False)
    assert collapse._grouped_route()
    new = collapse.batch_cluster_sequences(jobs)
    monkeypatch.setenv('CLH_NO_EDIT_MATRIX', '1')
    old = collapse.batch_cluster_sequences(jobs)
    monkeypatch.delenv('CLH_NO_EDIT_MATRIX')
    assert new == old and all(len(r) >= 1 for r in new)
    assert any(len(ids) > 1 for r in new for _, ids in r)                  # clusters were formed (K3 ran)
    raw = [[s for _, s in reads] for _, reads in jobs[:8]]
    groups = [[utils.compress_seq(s) for s in g] for g in raw]
    want = [utils.pairwise_distance(g) for g in groups]
    for got in (utils.pairwise_distance_groups(groups), utils.pairwise_distance_groups(raw, hpc=True)):
        assert len(got) == len(want)
        for a, b in zip(got, want):
            assert a.dtype == np.float64 and a.shape == b.shape and a.tobytes() == b.tobytes()
