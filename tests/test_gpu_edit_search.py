"""edlib.search on the GPU (K4s, csrc/edit_search.hip): every probe in every text, HW with locations.  The expected values are
always tests/edlib_check.py; one case also compares with the existing GPU path, edlib.align_batch over the written-out cross
product.  Edge lengths come from the plan's own geometry (EditSearchPlan.info), not from constants."""
import ctypes as C

import numpy as np
import pytest

import edit_search_check as chk

pytestmark = pytest.mark.gpu


def _ctx():
    from ciri_long_amd import hip
    return hip.default_context()


@pytest.fixture(scope='module')
def geom():
    plan = _ctx().edit_search_plan(['A'], ['A'])
    try:
        g = plan.info()
    finally:
        plan.close()
    assert g['seg'] >= 1 and g['round'] == 64 * g['seg'] and g['chunk'] % g['round'] == 0
    return g


def _check(probes, texts, k=-1, eq=None, both=False):
    from ciri_long_amd import edlib, utils
    got = edlib.search(probes, texts, k=k, both_strands=both, additionalEqualities=eq)
    assert got.shape == (len(texts), len(probes), 2 if both else 1) and got.dtype.names == ('distance', 'start', 'end', 'last_end', 'nlocs')
    for t, text in enumerate(texts):
        for p, probe in enumerate(probes):
            for s in range(got.shape[2]):
                want = chk.expected(utils.revcomp(probe) if s else probe, text, k, eq)
                assert chk.as_tuple(got[t, p, s]) == want, (t, p, s, len(probe), len(text))
    return got


@pytest.mark.parametrize('alpha', ['AC', 'ACGT'])
@pytest.mark.parametrize('lens', [(1, 2, 31, 32), (33, 63, 64)], ids=['word32', 'word64'])
def test_random_cross_products_on_the_length_grid(geom, lens, alpha):
    rng = chk.rng_for('gpu grid', lens, alpha)
    probes = [''.join(rng.choice(alpha) for _ in range(m)) for m in lens]
    texts = []
    for probe in probes:
        texts += [chk.random_text(rng, n, alpha, probe) for n in chk.text_lens(len(probe), geom['seg'])]
    _check(probes, texts)


def _planted(rng, n, probe, ends, alpha='CGT'):
    """n letters without the probe's letter 'A' ... with exact copies of the probe ending at the given columns"""
    t = [rng.choice(alpha) for _ in range(n)]
    for e in ends:
        t[e - len(probe) + 1:e + 1] = probe
    return ''.join(t)


@pytest.mark.parametrize('m', [20, 40], ids=['word32', 'word64'])
def test_planted_hits_at_the_edges_of_segments_rounds_and_waves(geom, m):
    rng = chk.rng_for('planted', m)
    seg, rnd, chunk = geom['seg'], geom['round'], geom['chunk']
    probe = 'A' + ''.join(rng.choice('ACGT') for _ in range(m - 2)) + 'A'
    n = 2 * rnd + 37
    cases = {
        'inside the first 2m columns': (n, [m - 1]),
        'a little later, still without a full warm-up': (n, [m + 3]),
        'ending at the last column': (n, [n - 1]),
        'straddling a segment boundary': (n, [5 * seg + m // 2]),
        'straddling a round boundary': (n, [rnd + m // 2]),
        'two equal hits in different segments': (n, [3 * seg + 2 + m, rnd + 11 * seg + 5]),
        'two equal hits in different rounds': (n, [rnd - 1, 2 * rnd + 30]),
        'straddling a wave boundary': (chunk + rnd + 5, [chunk + m // 2]),
        'two equal hits in different waves': (2 * chunk + 9, [chunk - 1, 2 * chunk + 8]),
    }
    texts = [_planted(rng, nn, probe, ends) for nn, ends in cases.values()]
    got = _check([probe], texts)
    for t, (name, (nn, ends)) in enumerate(cases.items()):
        assert chk.as_tuple(got[t, 0, 0]) == (0, ends[0] - m + 1, ends[0], ends[-1], len(ends)), name


def test_homopolymer_run_of_optimal_ends_is_counted_exactly(geom):
    seg, rnd, chunk = geom['seg'], geom['round'], geom['chunk']
    probes = ['A' * 7, 'A' * 33]
    texts = ['A' * (3 * seg + 1), 'A' * (rnd + 2 * seg + 3), 'C' * 50 + 'A' * (rnd + 5) + 'C' * 9, 'A' * (chunk + 70)]
    got = _check(probes, texts)
    for p, probe in enumerate(probes):
        m, n = len(probe), len(texts[1])
        assert chk.as_tuple(got[1, p, 0]) == (0, 0, m - 1, n - 1, n - m + 1)


def test_no_shared_letter_gives_the_probe_in_front_of_the_text(geom):
    probes = ['ACCA' * 5, 'AC' * 24]
    texts = ['G' * 5, 'GT' * (geom['round'] // 2 + 7)]
    got = _check(probes, texts)
    for p, probe in enumerate(probes):
        for t in range(len(texts)):
            # distance m, first found in front of the text; columns that m substitutions reach tie with it, as in align
            assert chk.as_tuple(got[t, p, 0])[:3] == (len(probe), 0, -1)


def test_k_keeps_a_best_of_k_and_drops_a_best_of_k_plus_one(geom):
    rng = chk.rng_for('k')
    probe = 'A' + ''.join(rng.choice('ACGT') for _ in range(28)) + 'A'
    hit = list(probe)
    for i in (4, 13, 22):
        hit[i] = 'C' if hit[i] != 'C' else 'G'
    text = _planted(rng, geom['round'] + 100, hit, [geom['round'] + 3])
    free = chk.expected(probe, text)
    assert free[0] == 3
    assert chk.as_tuple(_check([probe], [text], k=3)[0, 0, 0]) == free
    assert chk.as_tuple(_check([probe], [text], k=2)[0, 0, 0]) == (-1, -2, -2, -2, 0)


def test_both_strands_slot_one_is_the_reverse_complement(geom):
    from ciri_long_amd import edlib, utils
    rng = chk.rng_for('strands')
    probes = ['ACGGTTCAGGATTTACCGTA', 'GAATTCGAATTC', 'ACGT' * 9 + 'TTGCA']
    assert utils.revcomp(probes[1]) == probes[1]
    texts = []
    for n in (300, geom['round'] + 50):
        t = list(chk.random_text(rng, n, 'ACGT', probes[0]))
        t[40:40 + len(probes[2])] = utils.revcomp(probes[2])
        t[150:150 + len(probes[1])] = probes[1]
        texts.append(''.join(t))
    got = _check(probes, texts, both=True)
    single = edlib.search([utils.revcomp(p) for p in probes], texts)
    assert (got[:, :, 1] == single[:, :, 0]).all()
    assert (got[:, 1, 0] == got[:, 1, 1]).all()
    assert (got[:, 2, 1]['distance'] == 0).all() and (got[:, 2, 1]['start'] == 40).all()


def test_equalities_n_in_the_probe_matches_every_base(geom):
    rng = chk.rng_for('eq')
    eq = [('N', c) for c in 'ACGT']
    probes = ['ACGNNTGCATTGCANGT', 'N' * 5, 'ACGTTGCA' * 5 + 'NNNN' + 'GGATCC']
    texts = [chk.random_text(rng, n, 'ACGT', p.replace('N', 'G')) for n in (90, geom['round'] + 33) for p in probes]
    got = _check(probes, texts, eq=eq)
    assert (got[:, 1, 0]['distance'] == 0).all()
    plain = _check(probes, texts)
    assert (plain[:, 1, 0]['distance'] == 5).all()


def test_mixed_call_long_probes_empty_probe_and_empty_text(geom):
    rng = chk.rng_for('mixed')
    long65 = ''.join(rng.choice('ACGT') for _ in range(65))
    long200 = ''.join(rng.choice('ACGT') for _ in range(200))
    probes = ['ACGTTGCAAC', long65, '', long200, 'AC' * 30]
    texts = [chk.random_text(rng, 700, 'ACGT', long65), '', chk.random_text(rng, geom['round'] + 9, 'ACGT', long200), 'ACGTTGCAAC']
    _check(probes, texts)
    _check(probes, texts, k=4)
    _check(probes[:2], texts, both=True)


def test_equals_the_pair_route_over_the_written_out_cross_product(geom):
    from ciri_long_amd import edlib
    rng = chk.rng_for('pair route')
    probes = [''.join(rng.choice('ACGT') for _ in range(m)) for m in (12, 32, 33, 64)]
    texts = [chk.random_text(rng, n, 'ACGT', probes[i % 4]) for i, n in enumerate((50, geom['round'] - 1, geom['round'] + 1, 3 * geom['round'] + 17))]
    got = edlib.search(probes, texts, k=20)
    pairs = edlib.align_batch([p for _ in texts for p in probes], [t for t in texts for _ in probes], mode='HW', task='locations', k=20)
    for c, r in enumerate(pairs):
        locs = r['locations']
        want = (r['editDistance'], locs[0][0], locs[0][1], locs[-1][1], len(locs)) if locs else (r['editDistance'], -2, -2, -2, 0)
        assert chk.as_tuple(got[c // len(probes), c % len(probes), 0]) == want, c


def _raw(L, ctx, texts, toff, probes, poff, rows, cap):
    from ciri_long_amd import hip
    opts = hip.EditSearchOpts(-1, 0, None)
    return L.clh_edit_search_batch(ctx._h, len(toff) - 1, texts.ctypes.data, toff.ctypes.data, len(poff) - 1, probes.ctypes.data, poff.ctypes.data,
                                   C.byref(opts), rows.ctypes.data, cap)


def test_c_abi_argument_and_capacity_errors_and_a_plan_run_twice(geom):
    from ciri_long_amd import hip
    ctx, L = _ctx(), hip.lib()
    texts = np.frombuffer(b'ACGTACGTAC' * 3, dtype=np.uint8)
    probes = np.frombuffer(b'ACGTAC' + b'A' * 70, dtype=np.uint8)
    rows = np.zeros(4, dtype=hip.EDIT_SEARCH_DTYPE)
    ok_t, ok_p = np.array([0, 10, 30], dtype=np.int64), np.array([0, 4, 6], dtype=np.int64)
    assert _raw(L, ctx, texts, ok_t, probes, ok_p, rows, 4) == 0
    assert [chk.as_tuple(r) for r in rows] == [chk.expected(p, t) for t in ('ACGTACGTAC', 'ACGTACGTAC' * 2) for p in ('ACGT', 'AC')]
    assert _raw(L, ctx, texts, np.array([0, 20, 10], dtype=np.int64), probes, ok_p, rows, 4) == -2       # CLH_E_ARG
    assert _raw(L, ctx, texts, ok_t, probes, np.array([0, 5, 3], dtype=np.int64), rows, 4) == -2
    assert _raw(L, ctx, texts, ok_t, probes, np.array([0, 6, 71], dtype=np.int64), rows, 4) == -2        # a probe of 65 letters
    assert 'more than 64' in hip.last_error()
    assert _raw(L, ctx, texts, ok_t, probes, ok_p, rows, 3) == -4                                          # CLH_E_CAPACITY
    rng = chk.rng_for('twice')
    ps = ['ACGGTTCA', 'AC' * 20]
    ts = [chk.random_text(rng, n, 'ACGT', ps[0]) for n in (100, geom['chunk'] + 50)]
    plan = ctx.edit_search_plan(ps, ts)
    try:
        assert plan.info()['split_texts'] == 1
        plan.run()
        a = plan.fetch()
        plan.run()
        b = plan.fetch()
        assert plan.timing() > 0
    finally:
        plan.close()
    assert (a == b).all()
    for t in range(2):
        for p in range(2):
            assert chk.as_tuple(a[t, p]) == chk.expected(ps[p], ts[t])
