"""CPU statements to tests/splice_edges.py: every case reaches the edge it is named for -- read off the oracle's own trace
(oracle_lib.oracle_splice_trace, the body of clo_splice_signal with a record), never off the kernel --, K6's formulation
(tools/splice_scan_model.py: masks, packed key, lo / lo0 / hi_u / hi_d) equals the oracle on every case and on a seeded fuzz, the
Python statement of the step (ciri_long_amd/align.py) equals it too, and the sets have teeth: thirteen faults planted in the model are
each caught by the set named for it.

A case that misses its edge fails here; it does not become a weaker GPU test."""
import time

import numpy as np
import pytest

import oracle_lib
import splice_edges as E

M = E.M
K = M.constants()
_view = {}


def view(s, case):
    """the oracle's row and trace of a case as one dict, in the words of the cases' `expect`"""
    if case['label'] not in _view:
        row, tr = E.oracle_row(s, case, trace=True)
        v = dict(tr)
        v.update(row=row, us_free=row[1], ds_free=row[2], found=row[3], win=tuple(row[4:8]))
        _view[case['label']] = v
    return _view[case['label']]


def model_row(s, case, fault=0, _genomes={}):
    if s.name not in _genomes:
        _genomes[s.name] = (M.Genome(s.contigs), E.split_runs(*s.genome_runs()))
    g, sites = _genomes[s.name]
    return g.row(case['cand'], case['se'], case['st'], case['flags'], None if case['bare'] else sites, K, fault)


def one(name, label):
    s = E.build(name)
    found = [c for c in s.cases if c['label'] == '%s/%s' % (name, label)]
    assert len(found) == 1, (name, label)
    return s, found[0], view(s, found[0])


# ----------------------------------------------------------------------------------------------------------------------------
# the constants, the trace
# ----------------------------------------------------------------------------------------------------------------------------
def test_constants_are_parsed_from_the_kernel_source_and_a_missing_form_is_an_error(tmp_path):
    assert K['kWeight'] == [0, 1, 2, 2, 2] and len(K['kDonor']) == len(K['kAcceptor']) == 5
    # the tables are the reference's motifs in its order (align.py:32-45), as codes A0 C1 G2 T3
    for (donor, acceptor), d, a in zip(oracle_lib._SPLICE_MOTIFS, K['kDonor'], K['kAcceptor']):
        assert ('ACGT'.index(donor[0]), 'ACGT'.index(donor[1])) == d and ('ACGT'.index(acceptor[0]), 'ACGT'.index(acceptor[1])) == a
    assert [[n for n, _ in f] for f in K['KEY']] == [['clip_alt', 'alt', 'w'], ['alt', 'w', 'clip_alt'], ['w', 'alt', 'clip_alt']]
    assert K['FIELD_BITS'] == 15 and K['TIER_SHIFT'] == 60 and K['SLIDE_CAP'] == 100 and K['MASK_BITS'] == 64
    with open(M.SOURCE) as f:
        src = f.read()
    for gone in ('kWeight[5] = ', 'return key | (unsigned long long)tot;', 'use_anno && 2 * sl > 64)', 'for (int j = 1; j < 100; ++j)'):
        assert gone in src
        broken = tmp_path / 'broken.hip'
        broken.write_text(src.replace(gone, '/* moved */'))
        with pytest.raises(ValueError):
            M.constants(source=str(broken))


def test_the_search_bound_follows_from_the_field_width():
    """clh_device.h: kSpliceMaxSearch is the largest clip_base + search_extra at which alt <= us_len + ds_len still fits a key field"""
    import os
    import re
    with open(os.path.join(os.path.dirname(M.SOURCE), 'clh_device.h')) as f:
        dev = f.read()
    bits = int(re.search(r'static constexpr int kSpliceKeyBits = (\d+);', dev).group(1))
    cap = int(re.search(r'static constexpr int kSpliceSlideCap = (\d+);', dev).group(1))
    assert 'kSpliceMaxSearch = ((1 << kSpliceKeyBits) - 1 - 2 * (kSpliceSlideCap - 1)) / 2;' in dev
    assert bits == K['FIELD_BITS'] and cap == K['SLIDE_CAP']
    top = ((1 << bits) - 1 - 2 * (cap - 1)) // 2
    assert top == 16284
    field = (1 << bits) - 1
    for sl, fits in ((top, True), (top + 1, False)):
        us_len = ds_len = sl + cap - 1
        alt = us_len + ds_len                      # i = -us_len against j = ds_len
        # clip_alt = | alt - cb | <= max(alt, cb) and tot <= 2 max(sl, cap - 1) stay below alt's bound, w is at most 3
        assert (alt <= field) == fits and max(alt, sl) == alt and 2 * max(sl, cap - 1) <= alt
    # the key of the widest pair at the bound, packed by the source's own shifts, still holds every component apart
    sl, cb, free = top, 4096, cap - 1
    i, j = 1 - (sl + free), sl + free
    key = M.site_key(i, j, 3, cb, free, free, K)
    alt, tot = j - i, min(abs(i + free), abs(i - free)) + min(abs(j + free), abs(j - free))
    got = {name: (key >> shift) & field for name, shift in K['KEY'][2]}
    assert key >> K['TIER_SHIFT'] == 3 and got == {'w': 3, 'alt': alt, 'clip_alt': alt - cb} and key & field == tot and max(alt, tot) <= field
    with open(os.path.join(os.path.dirname(M.SOURCE), 'clh_api.hip')) as f:
        assert 'clip_base[i] + search_extra > clh::kSpliceMaxSearch' in f.read()


def test_the_trace_is_the_same_run():
    """clo_splice_trace's row equals clo_splice_signal's on every case (tests/test_splice_oracle.py pins the latter to the reference)"""
    n = 0
    for name in E.SETS:
        s = E.build(name)
        for c in s.cases:
            assert view(s, c)['row'] == E.oracle_row(s, c), c['label']
            n += 1
    assert n > 150


# ----------------------------------------------------------------------------------------------------------------------------
# every case reaches its edge
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', E.SETS)
def test_every_case_meets_what_it_is_named_for(name):
    s = E.build(name)
    offs = s.offsets()
    assert len(s.contigs) > 2 and all(len(t) <= 2048 for _, t in s.contigs)
    assert s.cases
    for c in s.cases:
        ctg = c['cand'][0]
        assert ctg != s.contigs[0][0] and offs[ctg] > 0 and offs[ctg] % 16 != 0, c['label']
        v = view(s, c)
        assert (v['us_free'], v['ds_free']) == E.slide(s.text(ctg), c['cand'][1], c['cand'][2]), c['label']      # the slide on the plain string
        for k, want in c['expect'].items():
            if k != 'status':
                assert v[k] == want, (c['label'], k, v[k], want)


def test_slide_edges():
    s = E.build('slide')
    got = {(view(s, c)['us_free'], view(s, c)['ds_free']) for c in s.cases}
    assert {(0, 0), (1, 0), (0, 1), (98, 98), (99, 99), (98, 99), (99, 98)} <= got
    # flanks of 99, 100 and 150 equal letters all give 99: the cap, not the text, stops them
    for up in (99, 100, 150):
        _s, c, v = one('slide', 'flanks %d/%d' % (up, up))
        t, (ctg, S, En, _cb, _h) = s.text(c['cand'][0]), c['cand']
        assert v['us_free'] == 99 and t[S - up:S] == t[En - up:En] and t[S:S + up] == t[En:En + up] and t[S - up - 1] != t[En - up - 1]
    # the contig's end stops the others: the letters would have gone on
    for label, side in (('E = L - 3', 'ds'), ('S = 3', 'us'), ('E == L', 'ds'), ('S == 0', 'us')):
        _s, c, v = one('slide', label)
        ctg, S, En, _cb, _h = c['cand']
        L = len(s.text(ctg))
        assert (En + v['ds_free'] == L) if side == 'ds' else (S - v['us_free'] == 0), label
    _s, c, v = one('slide', 'case only')
    t, (ctg, S, En, _cb, _h) = s.text(c['cand'][0]), c['cand']
    assert t[S - 3] == 'a' and t[En - 3] == 'A' and t[S - 6:S].upper() == t[En - 6:En].upper() and t[S:S + 6].upper() == t[En:En + 6].upper()
    _s, c, v = one('slide', 'IUPAC')
    t, (ctg, S, En, _cb, _h) = s.text(c['cand'][0]), c['cand']
    assert 'N' in t[S - 7:S] and 'n' in t[S:S + 7] and not set(t[S - 7:S + 7]) & set('ACGTacgt')


def test_contig_end_edges():
    s = E.build('contig_end')
    reached = set()
    for c in s.cases:
        ctg, S, En, cb, _h = c['cand']
        v, L, sl = view(s, c), len(s.text(ctg)), cb + c['se']
        head, tail = S - sl - v['us_free'] - 2, En + sl + v['ds_free'] + 2 - L
        # one side sits exactly on the rule (0 / -1 in front, L / L + 1 behind), the other well inside the contig
        assert (head in (0, -1) and tail < -100) or (head > 100 and tail in (0, 1)), (c['label'], head, tail)
        reached.add(('head', head) if head <= 0 else ('tail', tail))
        assert v['edge'] == (head < 0 or tail > 0) and v['anno'] == 1 - v['edge']
        # the annotated pair is there either way
        runs = E.split_runs(*s.contig_runs(ctg))
        assert S + 2 in runs[1] and En + 2 in runs[1]
    assert reached == {('head', 0), ('head', -1), ('tail', 0), ('tail', 1)}
    assert sorted(view(s, c)['found'] for c in s.cases) == [0, 1, 2, 2]


def test_slice_edges():
    s = E.build('slices')
    v = one('slices', 'wrapped, non-empty')[2]
    assert v['us'][2] == 1 and v['us'][1] > 0 and v['ds'][2] == 1 and v['ds'][3] == 1            # E - us_len < 0 wraps too
    assert one('slices', 'wrapped, empty')[2]['us'][1:3] == (0, 1)
    assert one('slices', 'start clamped')[2]['us'][2] == 2
    assert one('slices', 'end clipped')[2]['ds'][2:] == (0, 1)
    for tag in ('', ' (index)'):
        a, b = one('slices', 'len == need' + tag)[2], one('slices', 'len == need - 1' + tag)[2]
        assert a['ds'][1] == a['need'] and not a['short_seq'] and a['found'] and b['ds'][1] == b['need'] - 1 and b['short_seq']
        assert (a['ds'][2] == 1) == (tag == '')          # wrapped as a Python slice; from an index it ends with the contig
    v = one('slices', 'need <= 0')[2]
    assert v['need'] <= 0 and v['us'][1] == 0 and not v['short_seq'] and v['searched'] == {(0, 0), (0, 1)} and v['sites'] == 0
    for tag in ('', ' (index)'):
        for label, side, index in (('upstream index 0', 'us', 0), ('upstream index 1', 'us', 1), ('downstream index 0', 'ds', 0),
                                   ('downstream index 1', 'ds', 1)):
            _s, c, v = one('slices', label + tag)
            t = s.text(c['cand'][0])
            lo = v[side][0]
            assert t[lo + index:lo + index + 2] == ('AG' if side == 'us' else 'GT') and v['found'] == index
        _s, c, v = one('slices', 'both at n - 2' + tag)
        t = s.text(c['cand'][0])
        assert t[v['us'][0] + v['us'][1] - 2:][:2] == 'AG' and t[v['ds'][0] + v['ds'][1] - 2:][:2] == 'GT' and v['found'] == 1
    # served by an index, a start in front of the contig is no sequence at all
    for label in ('wrapped, non-empty', 'wrapped, empty', 'start clamped', 'need <= 0'):
        assert one('slices', label + ' (index)')[2]['us'][1] == -1


def test_mask_edges():
    s = E.build('masks')
    for strand in '+-':
        for kind in ('start', 'end'):
            hit = [one('masks', '%s %s at %d' % (strand, kind, sh))[2]['found'] for sh in (-15, 14, 15)]
            assert hit == [2, 2, 0]                         # g0 and g0 + span - 1 are shifts, g0 + span is not
    assert one('masks', 'cb 22 at 31')[1]['cand'][3] + 10 == 32          # 2 sl == 64: shift 31 is bit 63
    # cb = 23: handed back only where the annotation is consulted
    for label, status in (('cb 23', 1), ('cb 23, no sites loaded', 0), ('cb 23 at a contig end', 0)):
        _s, c, v = one('masks', label)
        assert 2 * (c['cand'][3] + c['se']) > K['MASK_BITS'] and model_row(s, c)[0] == status == c['expect']['status']
        assert (v['anno'] == 1) == (status == 1)
    # the neighbour's last position is this contig's offset: no window of a candidate that consults the annotation reaches it
    _s, c, v = one('masks', 'neighbour site at ctg_off')
    ctg, S, _e, cb, _h = c['cand']
    runs = E.split_runs(*s.genome_runs())
    assert all(s.offsets()[ctg] in r for r in runs) and S - (cb + 10) - v['us_free'] - 2 == 0 and v['shifts'][0][0] == []
    r = E.build('runs')
    cnt = r.genome_runs()[1].tolist()
    assert cnt[0] == 1 and cnt[1] >= 100000 and cnt[2] == cnt[3] == 0
    for cb in (5, 22):
        v = one('runs', 'every position, cb %d' % cb)[2]
        assert len(v['shifts'][0][1]) == 2 * (cb + 10) and len(v['shifts'][0][0]) == 2 * (cb + 10) + 1


def test_pair_edges():
    s = E.build('pairs')
    a, b = one('pairs', '|i - j| == T'), one('pairs', '|i - j| == T + 1')
    assert abs(a[2]['win'][1] - a[2]['win'][2]) == a[1]['cand'][3] + 3 and b[2]['shifts'][0] == ([-4], [5]) and b[2]['found'] == 0
    weights = [one('pairs', 'motif %d on %s' % (m, st))[2]['key'][2] for st in '+-' for m in range(5)]
    assert weights == [0, 1, 2, 2, 2] * 2
    for label in ('lower case', 'N', 'lower case on -'):
        assert one('pairs', label)[2]['key'][2] == 3
    _s, c, v = one('pairs', 'shift -sl joins')
    assert v['win'][1] == -(c['cand'][3] + 10) < 1 - v['us_len'] and v['found'] == 1 and v['anno'] == 1


def test_rank_edges():
    s = E.build('rank')
    duels = [c for c in s.cases if 'beats' in c]
    assert len(duels) >= 29
    seen = set()
    for c in duels:
        loser, field = c['beats']
        a, b = view(s, c), view(s, loser)
        assert a['sites'] == 2 and b['sites'] == 1, c['label']
        if field == 'tier':
            # the winner's tier is the lower one although the loser is the lighter site
            wa = a['key'][(2, 1, 0, 0)[a['tier']]]
            wb = b['key'][(2, 1, 0, 0)[b['tier']]]
            assert a['tier'] < b['tier'] and wa > wb, c['label']
        elif field == 'w':
            at = (2, 1, 0, 0)[a['tier']]
            assert a['tier'] == b['tier'] and [k for k in range(4) if a['key'][k] != b['key'][k]] == [at] and a['key'][at] < b['key'][at], c['label']
        else:
            assert a['tier'] == b['tier'], c['label']
            first = [k for k in range(4) if a['key'][k] != b['key'][k]]
            assert first and first[0] == field and a['key'][field] < b['key'][field], (c['label'], a['key'], b['key'])
            # a field after it favours the loser (but for tot, the last)
            assert field == 3 or any(a['key'][k] > b['key'][k] for k in range(field + 1, 4)), (c['label'], a['key'], b['key'])
        seen.add((a['tier'], field))
    # per tier: every adjacent pair of fields that can differ on their own, and tot as the last decider
    assert {(0, 0), (0, 2), (0, 3), (1, 0), (1, 1), (1, 3), (2, 0), (2, 1), (2, 3), (3, 0), (3, 1), (3, 3), (0, 'tier'), (1, 'tier'), (2, 'tier')} <= seen
    ties = [c for c in s.cases if c['expect'].get('same_key') == 2]
    assert len(ties) == 6 and {view(s, c)['found'] for c in ties} == {1, 2}


def test_what_cannot_be_reached_and_why():
    """edges one would list for the ranking and the contig ends that no input reaches"""
    for cb in range(0, 30):
        for i in range(-40, 41):
            for j in range(-40, 41):
                alt, clip_alt = abs(i - j), min(abs(j - i - cb), abs(j - i + cb))
                # clip_alt is a function of alt: among sites of equal alt it never decides, and in tier 0 (alt <= cb, clip_alt = cb - alt)
                # alt never decides after clip_alt
                assert clip_alt == abs(alt - cb)
                # a tier-2 site has i < 0 < j: with i == 0 or j == 0 inside its bounds alt <= cb, which is tier 0
                if -cb <= i <= 0 <= j <= cb and (i == 0 or j == 0):
                    assert alt <= cb
    # at a contig's start the upstream slice of an edge candidate wraps to the contig's end: the de-novo answer there is none unless
    # the contig is shorter than the two windows together (the slices set's wrapped cases)
    s, c, v = one('contig_end', 'S - sl - us_free - 2 == -1')
    assert v['us'][1:3] == (0, 1) and v['short_seq'] == 1


def test_strand_and_parameter_edges():
    s = E.build('strands')
    assert one('strands', 'host +, signal on -')[2]['searched'] == {(0, 0), (1, 1)}
    assert one('strands', 'host -, signal on +')[2]['searched'] == {(0, 1), (1, 0)}
    assert one('strands', 'canonical only, GC-AG present')[2]['found'] == 0 and one('strands', 'all motifs, GC-AG present')[2]['win'][3] == 1
    p = E.build('params')
    assert {(c['se'], c['st']) for c in p.cases} == {(0, 0), (1, 0), (10, 7)}
    assert {view(p, c)['found'] for c in p.cases} == {0, 1, 2}
    for c in p.cases:
        if c['label'].endswith('T apart') and 'T + 1' not in c['label'] and c['cand'][3] + c['se'] >= c['cand'][3] + c['st'] > 0:
            assert view(p, c)['found'] == 1, c['label']


# ----------------------------------------------------------------------------------------------------------------------------
# the model, the Python statement, the faults
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', E.SETS)
def test_model_and_python_statement_equal_the_oracle(name):
    s = E.build(name)
    for c in s.cases:
        want = view(s, c)['row']
        assert model_row(s, c) == E.kernel_row(c, want), c['label']
        if not c['flags'] & 2 and name != 'runs':
            assert E.mirror_row(s, c) == want, c['label']


def test_model_equals_the_oracle_on_a_seeded_fuzz():
    t0 = time.time()
    n, kinds, handed_back = 0, [0, 0, 0], 0
    for seed in range(36):
        se, st, flags = (0, 1, 10)[seed % 3], (0, 3, 7)[(seed // 3) % 3], seed % 4
        contigs, index, cands = E.fuzz_world(1000 + seed, 44, 14, clip_bases=(0, 1, 5, 20, 21, 22, 23), search_extra=se, fold=bool(flags & 2))
        g = M.Genome(contigs)
        lens = {name: len(t) for name, t in contigs}
        sites = E.split_runs(*E._runs(index, {name: g.span[name][0] for name in lens}, lens))
        texts = dict(contigs)
        runs = {name: E._runs({name: index.get(name, {})}, {name: 0}, lens) for name in lens}
        for c in cands:
            want = oracle_lib.oracle_splice_row(texts[c[0]], c[1], c[2], c[3], c[4], flags & 1, runs[c[0]], bool(flags & 2), se, st)
            got = g.row(c, se, st, flags, sites, K)
            if got[0] == 1 and want[0] == 0:            # cb = 23 with search_extra = 10, away from the contig ends: handed back, the slides kept
                L = lens[c[0]]
                assert 2 * (c[3] + se) > K['MASK_BITS'] and c[1] - (c[3] + se) - want[1] - 2 >= 0 and c[2] + (c[3] + se) + want[2] + 2 <= L
                assert got == [1, want[1], want[2], 0, 0, 0, 0, 0]
                handed_back += 1
                continue
            assert got == want, (seed, c, got, want)
            kinds[want[3]] += 1
            n += 1
    print('splice fuzz: %d cases (none %d, de novo %d, annotated pair %d), %d handed back, %.1f s' % (n, kinds[0], kinds[1], kinds[2], handed_back,
                                                                                                       time.time() - t0))
    assert n >= 20000 and handed_back >= 100 and min(kinds) >= 0.1 * n


@pytest.mark.parametrize('fault', M.FAULTS)
def test_each_planted_fault_is_caught_by_its_set(fault):
    s = E.build(E.FAULT_SET[fault])
    caught = [c['label'] for c in s.cases if model_row(s, c, fault) != E.kernel_row(c, view(s, c)['row'])]
    print('fault %d: %d of %d cases of %s differ' % (fault, len(caught), len(s.cases), s.name))
    assert caught, fault


def test_site_runs_as_the_host_flattens_them():
    """hip.flatten_splice_sites gives the runs the model reads; positions 0 and length + 1 are dropped, not aliased to a neighbour"""
    from ciri_long_amd import hip
    for name in ('masks', 'pairs'):
        s = E.build(name)
        flat, cnt = hip.flatten_splice_sites(s.index, s.offsets(), {n: len(t) for n, t in s.contigs})
        want = s.genome_runs()
        assert flat.tolist() == want[0].tolist() and cnt.tolist() == want[1].tolist()
    flat, cnt = hip.flatten_splice_sites({'b': {0: {'+': {'end': 1}}, 1: {'+': {'end': 1}}, 7: {'-': {'start': 1}}, 8: {'+': {'end': 1}, '-': {'start': 1}}}},
                                         {'a': 0, 'b': 5}, {'a': 5, 'b': 7})
    assert cnt.tolist() == [0, 1, 1, 0] and flat.tolist() == [6, 12]
    assert np.asarray(flat).dtype == np.int64
