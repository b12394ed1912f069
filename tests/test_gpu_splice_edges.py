"""K6 (splice_scan.hip) on the edge sets of tests/splice_edges.py: every row of Genome.splice_signals equals the row of
oracle/splice_oracle.c, all eight columns, no case left out.  tests/test_splice_edges_host.py proves from the oracle's trace that each
case reaches the edge it is named for, and that a kernel wrong in one of thirteen ways would give another row on these very sets."""
import numpy as np
import pytest

import oracle_lib
import splice_edges as E

pytestmark = pytest.mark.gpu

_oracle = {}


def want_rows(s):
    """the oracle's row per case of a set, computed once"""
    if s.name not in _oracle:
        _oracle[s.name] = [E.oracle_row(s, c) for c in s.cases]
    return _oracle[s.name]


def resident(s):
    from ciri_long_amd import hip
    dev = hip.Genome(hip.default_context(), s.contigs)
    assert [dev.offset[n] for n, _ in s.contigs] == [s.offsets()[n] for n, _ in s.contigs]
    return dev


def run_calls(dev, s, cases):
    """the cases through Genome.splice_signals, one call per (annotation or none, search_extra, shift_threshold, flags) -> rows by label"""
    groups = {}
    for c in cases:
        groups.setdefault((c['bare'], c['se'], c['st'], c['flags']), []).append(c)
    got = {}
    for (bare, se, st, flags), group in sorted(groups.items()):          # with the annotation first, then without
        dev.set_splice_sites(None if bare else (s.index or None))
        rows = dev.splice_signals([c['cand'] for c in group], se, st, bool(flags & 1), index_slices=bool(flags & 2))
        assert rows.shape == (len(group), 8) and rows.dtype == np.int32
        for c, r in zip(group, rows.tolist()):
            got[c['label']] = r
    return got


@pytest.mark.parametrize('name', E.SETS)
def test_every_set_equals_the_oracle(name):
    s = E.build(name)
    dev = resident(s)
    got = run_calls(dev, s, s.cases)
    dev.close()
    assert len(got) == len(s.cases)
    n_back = 0
    for c, want in zip(s.cases, want_rows(s)):
        assert got[c['label']] == E.kernel_row(c, want), (c['label'], c['cand'], got[c['label']], want)
        n_back += got[c['label']][0]
        if name in ('slide', 'contig_end', 'strands'):
            assert got[c['label']] == E.mirror_row(s, c), c['label']
    # nothing is handed back but the candidates past the masks
    assert n_back == sum(1 for c in s.cases if c['expect'].get('status') == 1)


@pytest.mark.parametrize('n', [1, 255, 256, 257])
def test_rows_do_not_depend_on_the_launch_geometry(n):
    """the rank set repeated to n candidates: one block less a lane, a full block, a block and one lane; equal candidates, equal rows"""
    s = E.build('rank')
    want = want_rows(s)
    dev = resident(s)
    dev.set_splice_sites(s.index)
    rows = dev.splice_signals([s.cases[k % len(s.cases)]['cand'] for k in range(n)], 10, 3, False).tolist()
    dev.close()
    assert len(rows) == n
    for k, r in enumerate(rows):
        assert r == want[k % len(s.cases)], (k, s.cases[k % len(s.cases)]['label'])


def test_invalid_candidates_get_status_1_and_leave_their_neighbours_alone():
    s = E.build('pairs')
    want = want_rows(s)
    dev = resident(s)
    dev.set_splice_sites(s.index)
    cands, expect = [], []
    for k, (c, w) in enumerate(zip(s.cases, want)):
        ctg, S, En, cb, host = c['cand']
        L = len(s.text(ctg))
        cands.append(c['cand']); expect.append(w)
        cands.append([(ctg, -1, En, cb, host), (ctg, En, En, cb, host), (ctg, S, L + 1, cb, host), (ctg, En, S, cb, host)][k % 4])
        expect.append([1, 0, 0, 0, 0, 0, 0, 0])
    rows = dev.splice_signals(cands, 10, 3, False).tolist()
    dev.close()
    assert rows == expect
    for c in cands[1::2]:
        assert oracle_lib.oracle_splice_row(s.text(c[0]), c[1], c[2], c[3], c[4], False, s.contig_runs(c[0])) == [1, 0, 0, 0, 0, 0, 0, 0]


def test_candidates_past_the_masks_get_the_python_answer_from_find_signal_batch():
    """cb = 23 (2 sl = 66 > 64) with annotation loaded: K6 hands the candidate back and align.find_signal_batch answers it with the
    Python statement; at a contig end the kernel answers itself"""
    from ciri_long_amd import align, env
    s = E.build('masks')
    cases = [c for c in s.cases if not c['bare']]
    host = E.TextGenome(s.contigs)
    env.initializer(None, host.contig_len, align.DeviceGenome(host, dict(s.contigs)), None, None, s.index)
    hosts = [{st: 1 for k, st in enumerate('+-') if (c['cand'][4] >> k) & 1} or None for c in cases]
    rows, extra = align.find_signal_rows([c['cand'][:4] for c in cases], hosts, False)
    got = align.find_signal_batch([c['cand'][:4] + (h,) for c, h in zip(cases, hosts)], False)
    env.GENOME.device.close()
    back = [c['label'] for c, r in zip(cases, rows.tolist()) if r[0] == 1]
    assert back == ['masks/cb 23'] and [k for k, v in extra.items() if v[0] == 'host'] == [cases.index(c) for c in cases if c['label'] == 'masks/cb 23']
    for c, g in zip(cases, got):
        ctg, S, En, cb, hm = c['cand']
        want = oracle_lib.oracle_splice_signal(s.text(ctg), S, En, cb, hm, False, s.contig_runs(ctg))
        assert g == want, (c['label'], g, want)
    assert got[[c['label'] for c in cases].index('masks/cb 23')][0] is not None
    # and the per-read Python path on the plain text
    env.initializer(None, host.contig_len, host, None, None, s.index)
    for c, h, g in zip(cases, hosts, got):
        ctg, S, En, cb, _hm = c['cand']
        site, us_free, ds_free, sig = align.find_annotated_signal(ctg, S, En, cb, cb + 10)
        if site is None:
            site = align.find_denovo_signal(ctg, S, En, h, sig, us_free, ds_free, cb, cb + 10, 3, False)
        assert g == (site, us_free, ds_free), c['label']


def test_small_contig_fuzz_in_one_call():
    """20 000 candidates on contigs of 3 to 1 200 letters in a single call; by the oracle alone each of none / de novo / annotated pair is at
    least a tenth of them"""
    contigs, index, cands = E.fuzz_world(4242, 400, 50)
    assert len(cands) == 20000
    lens = {n: len(t) for n, t in contigs}
    texts = dict(contigs)
    runs = {n: E._runs({n: index.get(n, {})}, {n: 0}, lens) for n in lens}
    want = [oracle_lib.oracle_splice_row(texts[c[0]], c[1], c[2], c[3], c[4], False, runs[c[0]]) for c in cands]
    kinds = [sum(1 for w in want if w[3] == k) for k in range(3)]
    print('fuzz shares: none %d, de novo %d, annotated pair %d' % tuple(kinds))
    assert sum(kinds) == 20000 and min(kinds) >= 2000 and all(w[0] == 0 for w in want)
    from ciri_long_amd import hip
    dev = hip.Genome(hip.default_context(), contigs)
    dev.set_splice_sites(index)
    rows = dev.splice_signals(cands, 10, 3, False).tolist()
    dev.close()
    assert len(rows) == 20000
    wrong = [(c, r, w) for c, r, w in zip(cands, rows, want) if r != w]
    assert not wrong, (len(wrong), wrong[:3])


def test_search_length_bound():
    """clip_base + search_extra up to 16284 (kSpliceMaxSearch: alt <= us_len + ds_len still fits a 15-bit key field) is answered, one
    more is refused.  One motif occurrence per window; both windows are the whole contig."""
    from ciri_long_amd import hip
    s = E.build('slide')
    c = [k for k in s.cases if k['label'] == 'slide/flanks 1/1'][0]
    ctg, S, En, _cb, _h = c['cand']
    dev = resident(s)
    for sl in (16283, 16284):
        row = dev.splice_signals([(ctg, S, En, 4096, 0)], sl - 4096, 3, False).tolist()[0]
        want = oracle_lib.oracle_splice_row(s.text(ctg), S, En, 4096, 0, False, None, False, sl - 4096, 3)
        assert row == want and row[3] == 1, (sl, row, want)
    with pytest.raises(hip.ClhError, match=r'clip_base \+ search_extra above 16284'):
        dev.splice_signals([(ctg, S, En, 4096, 0)], 16285 - 4096, 3, False)
    with pytest.raises(hip.ClhError, match=r'clip_base \+ search_extra above 16284'):
        dev.splice_signals([(ctg, S, En, 0, 0)], 16285, 3, False)
    dev.close()


def test_refusals_carry_their_messages():
    from ciri_long_amd import hip
    s = E.build('pairs')
    c = s.cases[0]['cand']
    dev = resident(s)
    for cb in (-1, 4097):
        with pytest.raises(hip.ClhError, match='clip_base out of range'):
            dev.splice_signals([(c[0], c[1], c[2], cb, 0)])
    assert dev.splice_signals([(c[0], c[1], c[2], 4096, 0)]).shape == (1, 8)
    with pytest.raises(hip.ClhError, match='negative search length'):
        dev.splice_signals([c], -1, 3)
    with pytest.raises(hip.ClhError, match='negative search length'):
        dev.splice_signals([c], 10, -1)
    total = sum(len(t) for _, t in s.contigs)
    cols = {'ctg_off': [total - 10], 'ctg_len': [11], 'start': [1], 'end': [5], 'clip_base': [5], 'host_mask': [0]}
    with pytest.raises(hip.ClhError, match='contig outside the genome'):
        dev.splice_signals(cols)
    cols['ctg_off'] = [-1]
    with pytest.raises(hip.ClhError, match='contig outside the genome'):
        dev.splice_signals(cols)
    for bad in ([5, 5, 9], [9, 5, 7], [3, total + 1, total + 2]):
        pos = np.array(bad, dtype=np.int64)
        cnt = np.array([3, 0, 0, 0], dtype=np.int64)
        assert hip.lib().clh_genome_set_splice_sites(dev._h, pos.ctypes.data, cnt.ctypes.data) != 0
        assert 'positions must be strictly ascending and inside the genome' in hip.last_error()
    # two runs may hold the same position; a run must not hold it twice
    pos = np.array([5, 9, 5, 9], dtype=np.int64)
    cnt = np.array([2, 2, 0, 0], dtype=np.int64)
    assert hip.lib().clh_genome_set_splice_sites(dev._h, pos.ctypes.data, cnt.ctypes.data) == 0
    # flatten_splice_sites drops positions 0 and length + 1 of a contig: they would be the neighbours' sites
    ctg, S, En, cb, _h = c
    L = len(s.text(ctg))
    index = {ctg: dict(s.index[ctg])}
    index[ctg][0] = {'+': {'end': 1, 'start': 1}}
    index[ctg][L + 1] = {'+': {'end': 1, 'start': 1}}
    flat, cnt = hip.flatten_splice_sites(index, dev.offset, dev.length)
    kept, cnt0 = hip.flatten_splice_sites({ctg: s.index[ctg]}, dev.offset, dev.length)
    assert flat.tolist() == kept.tolist() and cnt.tolist() == cnt0.tolist()
    dev.set_splice_sites(index)
    assert dev.splice_signals([c], 10, 3, False).tolist()[0] == want_rows(s)[0]
    dev.close()
