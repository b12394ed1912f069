"""CPU statements to tests/ccs_edges.py: the constants are the ones the sources state, every case reaches the edge it is named for --
read off the oracle's own trace (oracle_lib.oracle_ccs_trace, the body of clo_ccs_segments with a record), never off the kernel --,
K2's formulation (tools/ccs_scan_model.py: chains, strided maxima, butterflies, guarded anchor search) equals clo_ccs_segments plus
the tail rule over a grid of thread counts, bucket counts and insertion orders, and the sets have teeth: nine one-line faults planted
in the model's source are each caught by a named set.

A case that misses its edge fails here; it does not become a weaker GPU test."""
import os

import numpy as np
import pytest

import ccs_edges as E
import oracle_lib

M = E.M
K = E.constants()
DMIN, SMOOTH, GUARD, CAP, TAIL = K['CCS_DMIN'], K['CCS_SMOOTH'], K['CCS_GUARD'], K['CCS_MAX_CUTS'], K['CCS_MIN_TAIL']

_cases, _trace = {}, {}


def cases_of(name):
    if name not in _cases:
        _cases[name] = E.SETS[name](K)
        assert _cases[name], name
    return _cases[name]


def trace(case):
    key = case.read.tobytes()
    if key not in _trace:
        _trace[key] = oracle_lib.oracle_ccs_trace(case.read)
    return _trace[key]


def one(name, **what):
    """the case of a set whose `what` holds these items"""
    found = [c for c in cases_of(name) if all(c.what.get(k) == v for k, v in what.items())]
    assert len(found) == 1, (name, what, len(found))
    return found[0], trace(found[0])


# ----------------------------------------------------------------------------------------------------------------------------
# the constants, the trace
# ----------------------------------------------------------------------------------------------------------------------------
def test_constants_are_parsed_from_the_sources_and_a_missing_one_is_an_error(tmp_path):
    for name in M._INTS + ('kK2LdsMax', 'CCS_SEG_CAP'):
        assert isinstance(K[name], int) and K[name] > 0, name
    assert K['T'][0] == K['K2_WIDE_FROM'] and list(K['T']) == sorted(K['T']) and all(t % 64 == 0 for t in K['T'])
    assert [M.k2_buckets(x, K) for x in (64, 1536, 1537, 3072, 3073, 16000)] == [512, 512, 1024, 1024, 2048, 2048]
    with open(M.SOURCE) as f:
        src = f.read()
    moved = tmp_path / 'moved.hip'
    moved.write_text(src.replace('K2_WIDE_FROM = %d;' % K['K2_WIDE_FROM'], 'K2_WIDE_FROM = 2048;').replace('lcap <= 1536 ? 512', 'lcap <= 1280 ? 512'))
    K2 = M.constants(source=str(moved))
    assert K2['K2_WIDE_FROM'] == 2048 and E.class_lengths(K2)[:7] == [1984, 1985, 2047, 2048, 2049, 1280, 1281]
    for gone in ('CCS_MIN_TAIL = ', 'inline int k2_buckets(int lcap) { return', 'K2_LDS_MAX = '):
        assert gone in src
        broken = tmp_path / 'broken.hip'
        broken.write_text(src.replace(gone, gone.replace('= ', '=  ').replace('return', 'return  ')))
        with pytest.raises((KeyError, ValueError)):
            M.constants(source=str(broken))
    with open(M.API) as f:
        api = f.read()
    broken = tmp_path / 'broken_api.hip'
    broken.write_text(api.replace('static const int T[] = {', 'static const int T[] = { /* */'))
    with pytest.raises(ValueError):
        M.constants(api=str(broken))


def test_the_trace_is_the_run_of_clo_ccs_segments_and_counts_what_it_says():
    for name in E.SETS:
        for c in cases_of(name):
            t = trace(c)
            assert (t['period'], t['cuts'], t['support'] if t['period'] else 0) == oracle_lib.oracle_ccs_segments(c.read), (name, c.what)
            if t['best'] >= K['CCS_MIN_SUPPORT']:
                # the exit `n < 2` behind the cuts is never taken: bestd <= L/2 and p0 <= bestd leave room for a second cut
                assert t['period'] == t['p0'] > 0 and len(t['cut']) >= 2 and t['p0'] <= t['bestd'] <= len(c.read) // 2, (name, c.what)
            for row in t['cut']:
                assert row['lo'] <= row['v'] <= row['hi'] and row['score_tied'] >= row['score_dist_tied'] >= 1
                assert (row['score'] > 0) == bool(row['anchor_ran'])
                if row['anchor_ran']:
                    assert row['dist_tied'] >= row['i_tied'] >= row['a_tied'] >= 1 and abs(row['delta'] - row['v']) <= GUARD
    # a read small enough to count by hand: 19 bases occur again 50 later -> 12 pairs at offset 50, smoothed over 47..53
    c, t = one('thresholds', support=K['CCS_MIN_SUPPORT'])
    r = c.read
    assert sum(1 for i in range(len(r) - 57) if (r[i:i + 8] == r[i + 50:i + 58]).all()) == 12
    assert (t['bestd'], t['best'], t['tied']) == (47, 12, 7) and t['harmonics'] == []          # (47 + 1) / 2 < CCS_DMIN: no harmonic is evaluated


# ----------------------------------------------------------------------------------------------------------------------------
# every case reaches its edge
# ----------------------------------------------------------------------------------------------------------------------------
def test_classes_lie_on_both_sides_of_every_routing_boundary():
    cs = cases_of('classes')
    lengths = [len(c.read) for c in cs]
    assert lengths == [960, 961, 1023, 1024, 1025, 1536, 1537, 3072, 3073, 16000, 16001, 16500]
    alone = [M.route(L, [L], K) for L in lengths]
    assert alone == [('one wave', 512)] + [('x4', 512)] * 5 + [('x4', 1024)] * 2 + [('x4', 2048)] * 2 + [('long', 2048)] * 2
    mixed = [M.route(L, lengths, K) for L in lengths]
    assert mixed == [('x4', 512)] * 6 + alone[6:]                     # beside a longer read the 960 bases are filed under 1024
    assert [M.route(L, lengths, K, one_wave=True)[0] for L in lengths] == ['one wave'] * 10 + ['long'] * 2
    assert sorted(E.mixed_order(len(cs))) == list(range(len(cs))) and E.mixed_order(len(cs)) != list(range(len(cs)))
    for c in cs:
        t = trace(c)
        assert t['period'] > 0 and t['tied'] == 7 and c.what['long'] == (len(c.read) > K['kK2LdsMax'])
    assert any(len(c.read) % 2 for c in cs) and trace(cs[-1])['period'] != trace(cs[-2])['period']
    assert len(trace(cs[-1])['cuts']) == len(trace(cs[-2])['cuts']) == CAP          # the long kernel's reads run into the cap


def test_thresholds_are_met_and_missed_by_one():
    sup = K['CCS_MIN_SUPPORT']
    c, t = one('thresholds', support=sup)
    assert t['best'] == t['support'] == sup and t['period'] == 47 and len(t['cuts']) >= 2
    c, t = one('thresholds', support=sup - 1)
    assert t['best'] == sup - 1 and t['period'] == 0
    c, t = one('thresholds', length=2 * DMIN - 1)
    assert len(c.read) == 2 * DMIN - 1 and t['period'] == 0
    c, t = one('thresholds', length=2 * DMIN)
    assert len(c.read) == 2 * DMIN and (t['period'], t['cuts'], t['bestd']) == (DMIN, [DMIN, 2 * DMIN], len(c.read) // 2)
    c, t = one('thresholds', two_copies=200)
    assert (t['period'], t['cuts']) == (97, [100, 200])
    for what in ({'two_copies': 199}, {'few_cuts': True}):
        c, t = one('thresholds', **what)
        assert t['period'] == 0 and t['best'] == 0           # the repeat's offset lies above L/2: nothing is counted


def test_periods_at_the_limits():
    c, t = one('period limits', multiple=True)
    assert t['bestd'] == 2 * (DMIN - 1) - SMOOTH and all(x % (DMIN - 1) == 0 for x in t['cuts']) and t['harmonics'] == []
    for c in cases_of('period limits'):
        t = trace(c)
        if c.what.get('clipped_at_dmin'):
            assert t['period'] > 0 and t['bestd'] - SMOOTH < DMIN <= t['bestd'], c.what         # the best offset's own sum is clipped below
            assert (t['tied'] < 2 * SMOOTH + 1) == (c.what['unit'] - SMOOTH < DMIN)
        if 'extra' in c.what:
            dmax = len(c.read) // 2
            assert t['period'] == 97 and t['best'] == len(c.read) - 100 - 7            # every pair at d = 100 counts, also where 100 == dmax
            assert (c.what['unit'] + SMOOTH > dmax) == c.what['clipped_at_dmax'] == (t['tied'] < 2 * SMOOTH + 1)
    c, t = one('period limits', last_kmer=True)
    r = c.read
    assert (r[len(r) - 58:len(r) - 50] == r[len(r) - 8:]).all() and t['best'] == K['CCS_MIN_SUPPORT'] and t['period'] == 47
    c, t = one('period limits', last_kmer=False)
    assert t['best'] == K['CCS_MIN_SUPPORT'] - 1 and t['period'] == 0


def test_plateaus_lie_across_lanes_strides_and_waves():
    crossed = set()
    for c in cases_of('plateaus'):
        t = trace(c)
        p = c.what['unit']
        assert t['tied'] == 2 * SMOOTH + 1 and t['bestd'] == t['period'] == p - SMOOTH, c.what        # seven equal maxima, the smallest reported
        assert c.what['lanes64'] == [(d - DMIN) % 64 for d in range(p - SMOOTH, p + SMOOTH + 1)]
        assert 63 in c.what['lanes64'] and 0 in c.what['lanes64']
        l256 = c.what['lanes256']
        crossed |= {w for w in (64, 128, 192) if w - 1 in l256 and w in l256} | ({256} if 255 in l256 and 0 in l256 else set())
    assert crossed == {64, 128, 192, 256}
    assert len({len(c.read) for c in cases_of('plateaus') if c.what['unit'] == E.plateau_periods(K)[0]}) == 3


def test_harmonics_at_a_margin_of_zero_and_minus_one():
    c, t = one('harmonics', margin=0)
    h = t['harmonics'][0]
    assert (h['q'], h['margin']) == (2, 0) and t['period'] == h['e'] and t['bestd'] > 2 * h['e'] - 4
    c, t = one('harmonics', margin=-1)
    h = t['harmonics'][0]
    assert (h['q'], h['margin']) == (2, -1) and t['period'] == t['bestd']
    c, t = one('harmonics', q=3)
    h = {x['q']: x for x in t['harmonics']}
    assert h[2]['margin'] < 0 <= h[3]['margin'] and t['period'] == h[3]['e'] and all(h[q]['margin'] < 0 for q in h if q > 3)
    c, t = one('harmonics', evaluated=2)
    assert [x['q'] for x in t['harmonics']] == [2, 3] and (t['bestd'] + 2) // 4 < DMIN


def test_cuts_at_the_cap_the_tail_and_the_tolerances():
    for c in cases_of('cuts'):
        t, w = trace(c), c.what
        segs = E.want_of(c.read, K)['segs']
        if 'ncuts' in w:
            assert len(t['cuts']) == w['ncuts'], w
        if 'tail' in w:
            assert (len(segs) == len(t['cuts']) + 1) == w['tail'], w
        if 'tol' in w:
            assert t['p0'] == w['p0'] and t['cut'][0]['lo'] == w['p0'] - w['tol'] and t['cut'][0]['hi'] == w['p0'] + w['tol']
        if 'W' in w:
            assert t['p0'] == w['p0'] and min(t['p0'], 96) == w['W']
        assert t['cut'][0]['b'] == 0                                   # the first window is clipped at 0
    short = [c for c in cases_of('cuts') if c.what.get('copies') == CAP - 1]
    assert sorted(len(c.read) - trace(c)['cuts'][-1] for c in short) == [0, TAIL - 1, TAIL]
    capped = [c for c in cases_of('cuts') if c.what.get('ncuts') == CAP]
    assert sorted(len(c.read) - trace(c)['cuts'][-1] for c in capped) == [0, TAIL, 40]        # 20 and 40 bases left behind the cap: no tail
    c, t = one('cuts', last=85)
    assert t['cut'][-1]['lo'] == t['cut'][-1]['hi'] == 85 == len(c.read) - t['cut'][-1]['b'] and t['cut'][-1]['anchor_ran'] == 0
    assert t['cut'][-1]['b'] + min(t['p0'], 96) > len(c.read)          # ... and the last one at L
    c, t = one('cuts', last=84)
    assert len(c.read) - t['cuts'][-1] == t['cut'][0]['lo'] - 1


def test_vote_ties_and_windows_without_anchors():
    for c in cases_of('vote'):
        t, w = trace(c), c.what
        if 'tie' in w:
            row = t['cut'][w['cut']]
            prev = t['cut'][w['cut'] - 1]['delta'] if w['cut'] else t['p0']
            assert row['score_tied'] == 2 and row['v'] == w['v'], w
            a, b = w['between']
            assert row['score_dist_tied'] == (2 if w['tie'] == 'delta' else 1) and (abs(a - prev) == abs(b - prev)) == (w['tie'] == 'delta')
    c, t = one('vote', tie='distance', cut=2)
    assert t['cut'][2]['v'] == 100 == t['cut'][1]['delta']              # the larger offset wins by its distance from prev
    c, t = one('vote', no_anchor=(2, 3))
    for n in (2, 3):
        row = t['cut'][n]
        assert row['score'] == 0 and not row['anchor_ran'] and row['delta'] == t['cut'][n - 1]['delta'] and row['score_tied'] == row['hi'] - row['lo'] + 1
        i0, i1 = max(0, row['b'] - 96), row['b'] + 96
        assert all((c.read[i:i + 8] == 4).any() for i in range(i0, i1))
    c, t = one('vote', beyond_guard=2)
    row = t['cut'][2]
    i = row['b'] - 4
    assert max(4, t['p0'] // 8) > GUARD and (c.read[i:i + 8] == c.read[i + 109:i + 117]).all() and row['lo'] <= 109 <= row['hi']
    assert (row['v'], row['delta'], row['dist']) == (100, 100, 5) and 109 - row['v'] > GUARD


def test_anchor_keys_are_each_decisive_once():
    c, t = one('anchor keys', key=2)
    row = t['cut'][2]
    assert (row['dist_tied'], row['i_tied']) == (2, 1) and (row['i'], row['delta'], row['dist']) == (c.what['i'], c.what['delta'], 5)
    assert row['i'] == row['b'] + 1 and (c.read[row['b'] - 9:row['b'] - 1] == c.read[row['b'] + 91:row['b'] + 99]).all()       # the loser: b - 9 at offset p
    c, t = one('anchor keys', key=3)
    row = t['cut'][2]
    assert (row['dist_tied'], row['i_tied'], row['a_tied']) == (3, 3, 1) and row['delta'] == 80 == t['cut'][1]['delta'] and row['i'] == c.what['i']
    assert all((c.read[row['i']:row['i'] + 8] == c.read[row['i'] + d:row['i'] + d + 8]).all() for d in (75, 80, 85))
    c, t = one('anchor keys', key=4)
    row = t['cut'][2]
    assert (row['dist_tied'], row['i_tied'], row['a_tied']) == (2, 2, 2) and row['delta'] == 75 and t['cut'][1]['delta'] == 80
    assert [bool((c.read[row['i']:row['i'] + 8] == c.read[row['i'] + d:row['i'] + d + 8]).all()) for d in (75, 80, 85)] == [True, False, True]


def test_n_and_codes_outside_the_alphabet():
    from ciri_long_amd import hip
    c, t = one('N and odd codes', N='first and last')
    assert c.read[0] == c.read[-1] == 4 and t['period'] == 87
    c, t = one('N and odd codes', N='every 8th of a copy')
    a, b = c.what['copy']
    assert all((c.read[i:i + 8] == 4).any() for i in range(a, b - 8)) and t['period'] == 87
    c, t = one('N and odd codes', N='all')
    assert (c.read == 4).all() and t['best'] == 0 and t['period'] == 0
    c, t = one('N and odd codes', odd=(100, 291))
    data, off = hip.pack([c.read])                 # hip.pack lets any int8 through; K2 and the oracle read it as "not 0..3"
    assert (data[100], data[291]) == (7, -3) and t['period'] == 87 and t['best'] < trace(cases_of('N and odd codes')[0])['best']


def test_chains_hold_every_position_or_many_codes():
    for c in cases_of('chains'):
        st = {}
        got = M.scan(c.read, 64, 512, 'ascending', K, stats=st)
        want = oracle_lib.oracle_ccs_segments(c.read)
        assert (got[0], got[3], got[2]) == want, c.what
        n = len(c.read) - 7
        assert len(c.read) == E.LOW_COMPLEXITY
        if 'chains' in c.what:
            assert st['longest_chain'] == -(-n // c.what['chains']) and st['unequal_visits'] == 0, (c.what, st)
        else:
            print('few buckets: longest chain %d, %d visits of another code' % (st['longest_chain'], st['unequal_visits']))
            assert st['unequal_visits'] > n and st['longest_chain'] > 8


# ----------------------------------------------------------------------------------------------------------------------------
# the model equals the oracle
# ----------------------------------------------------------------------------------------------------------------------------
# The model's time goes with its chain steps: M.cost for the period count, and per cut two walks of 2 W window positions over chains of
# about 2 cost / L.  CASE_STEPS bounds one (case, grid point), SET_STEPS the grid points of one set, cheapest cases first: the whole file
# takes about 20 s.  What falls outside is printed by the test: mostly the grid points with ONE bucket (a single chain of L positions)
# of reads above about 450 bases, every grid point of the classes from 3072 bases on, and all but the kernel's own bucket count for
# the three low-complexity reads of 1100 bases.  test_every_case_in_the_kernels_own_configuration runs EVERY case with the buckets of
# its class at NT 64, and at NT 256 as well unless the read is one of the long kernel's or low-complexity.
GRID = [(nt, nb, order) for nt in (1, 3, 64, 256) for nb in (1, 512, 2048) for order in ('ascending', 'descending')]
CASE_STEPS = 1500000
SET_STEPS = 12000000


def steps(case, nb):
    t = trace(case)
    c = M.cost(case.read, nb, K)
    L = max(len(case.read), 1)
    return c + len(t['cut']) * 4 * min(max(t['p0'], 1), 96) * (2 * c // L + 1)


def model_answer(read, nt, nb, order, scan=M.scan):
    rec = scan(read, nt, nb, order, K)
    return rec[0], M.segments(len(read), rec, K)


def oracle_answer(case):
    w = E.want_of(case.read, K)
    return w['period'], w['segs']


@pytest.mark.parametrize('name', list(E.SETS))
def test_model_equals_the_oracle_over_threads_buckets_and_orders(name):
    total, ran, outside = 0, 0, []
    for c in sorted(cases_of(name), key=lambda c: steps(c, 1)):
        for nt, nb, order in GRID:
            s = steps(c, nb)
            if s > CASE_STEPS or total + s > SET_STEPS:
                outside.append((len(c.read), nt, nb, order))
                continue
            total += s
            ran += 1
            assert model_answer(c.read, nt, nb, order) == oracle_answer(c), (name, c.what, nt, nb, order)
    print('%s: %d grid points, %d outside the budget (reads of %s bases)' % (name, ran, len(outside), sorted({x[0] for x in outside})))
    assert ran >= 2 * len(GRID) // 3          # at least one case at every grid point but those of one bucket


@pytest.mark.parametrize('name', list(E.SETS))
def test_every_case_in_the_kernels_own_configuration(name):
    for c in cases_of(name):
        L = len(c.read)
        nb = M.route(L, [L], K)[1]
        for nt in ((64,) if L > K['kK2LdsMax'] or M.cost(c.read, nb, K) > 200000 else (64, 256)):
            assert model_answer(c.read, nt, nb, 'ascending') == oracle_answer(c), (name, c.what, nt)


# ----------------------------------------------------------------------------------------------------------------------------
# the sets have teeth
# ----------------------------------------------------------------------------------------------------------------------------
# (name, text of tools/ccs_scan_model.py, what replaces it, the set that must catch it)
MUTANTS = [
    ('the chain walk does not compare the codes', 'if code[j] == ci:', 'if code[j] == ci or True:', 'chains'),
    ('a pair at d = dmax is not counted', 'if d >= DMIN and d <= dmax:', 'if d >= DMIN and d < dmax:', 'period limits'),
    # cnt exists over [DMIN, L/2] alone; the kernel's array happens to hold zeros below DMIN, so there the fault reads memory the
    # formulation does not own instead of giving a wrong number: the model answers it with a KeyError, which counts as caught
    ('the smoothing is not clipped at DMIN', 'lo = max(d - SMOOTH, DMIN)', 'lo = d - SMOOTH', 'period limits'),
    ('the period merge keeps any of equal maxima', 'return b2 > best or (b2 == best and d2 < bestd)', 'return b2 > best', 'plateaus'),
    ('the vote merge has no distance key', 'return s2 > bs or (s2 == bs and (t2 < bdist or (t2 == bdist and e2 < bdel)))',
     'return s2 > bs or (s2 == bs and e2 < bdel)', 'vote'),
    ('the anchor search runs over the whole tolerance', 'glo, ghi = max(bdel - GUARD, dlo), min(bdel + GUARD, dhi)', 'glo, ghi = dlo, dhi', 'vote'),
    ('closer prefers the smaller i', '(i2 > i1_ or', '(i2 < i1_ or', 'anchor keys'),
    ('closer has no third key', '(i2 == i1_ and (a2 < a1 or (a2 == a1 and e2 < e1)))', '(i2 == i1_ and e2 < e1)', 'anchor keys'),
    ('the tail is kept at the cap', "tail = L - b >= K['CCS_MIN_TAIL'] and ncuts < K['CCS_MAX_CUTS']", "tail = L - b >= K['CCS_MIN_TAIL']", 'cuts'),
]


def _mutant(old, new):
    path = os.path.abspath(M.__file__.replace('.pyc', '.py'))
    with open(path) as f:
        src = f.read()
    assert src.count(old) == 1, (old, src.count(old))
    ns = {'__name__': 'ccs_scan_model_mutant', '__file__': path}
    exec(compile(src.replace(old, new), path, 'exec'), ns)
    return ns


def _caught_by(ns, case):
    """the kernels' two thread counts at the buckets of the read's class"""
    nb = M.route(len(case.read), [len(case.read)], K)[1]
    for nt in (64, 256):
        try:
            rec = ns['scan'](case.read, nt, nb, 'ascending', K)
            if (rec[0], ns['segments'](len(case.read), rec, K)) != oracle_answer(case):
                return True
        except (KeyError, IndexError):
            return True
    return False


@pytest.mark.parametrize('name,old,new,by', MUTANTS, ids=[m[0] for m in MUTANTS])
def test_a_planted_fault_in_the_model_is_caught_by_a_named_set(name, old, new, by):
    ns = _mutant(old, new)
    catching = [c.what for c in sorted(cases_of(by), key=lambda c: steps(c, 512)) if steps(c, 512) <= CASE_STEPS and _caught_by(ns, c)][:3]
    print('%s: caught by %s %s' % (name, by, catching))
    assert catching, name


def test_the_unchanged_source_passes_where_the_mutants_fail():
    ns = _mutant('def scan(', 'def scan(')
    for by in ('plateaus', 'vote', 'anchor keys'):
        assert not any(_caught_by(ns, c) for c in cases_of(by))
