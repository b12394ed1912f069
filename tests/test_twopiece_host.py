"""Two-piece affine gap costs on the CPU: the definition (tests/twopiece_check.py) against the enumeration of every alignment,
against itself (cell by cell and row by row), against the one-piece checkers where the second piece is dominated, and the scheme
of the kernel (tools/twopiece_model.py) against the definition -- which is where the argument about the scan's missing cross term is
held -- with planted faults that named case sets catch."""
import itertools
import os
import sys

import numpy as np
import pytest

import anchored_check as ac
import ends_check as ec
import twopiece_check as chk

TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools')
sys.path.insert(0, TOOLS)
import twopiece_model as mdl  # noqa: E402

SMALL_COSTS = [(3, 2, 6, 1), (2, 2, 2, 2), (1, 1, 3, 0), (0, 0, 0, 0)]
MAT = chk.dna_matrix(2, 4)


def _small_words(max_len=4, alphabet='AC', min_len=1):
    return [''.join(w) for n in range(min_len, max_len + 1) for w in itertools.product(alphabet, repeat=n)]


# ---- the enumeration: every alignment of a shape, as its M cells and its maximal gap runs ---------------------------------------
def _paths(mode, m, n):
    """every alignment the mode admits for an m x n pair -> [(start, end, M cells, gap run lengths)]; ops in every order, a maximal
    run of one op is one gap"""
    anchored = mode in ('global', 'prefix', 'extend')
    if anchored:
        starts = [(0, 0)]
    elif mode == 'semiglobal':
        starts = [(0, j) for j in range(n + 1)]
    else:
        starts = [(0, j) for j in range(n + 1)] + [(i, 0) for i in range(1, m + 1)]

    def is_end(i, j):
        if mode == 'global':
            return (i, j) == (m, n)
        if mode in ('semiglobal', 'prefix'):
            return i == m
        if mode == 'overlap':
            return i == m or j == n
        return True
    out = []

    def go(i, j, start, cells, runs, last):
        if is_end(i, j):
            out.append((start, (i, j), tuple(cells), tuple(runs)))
        if i < m and j < n:
            go(i + 1, j + 1, start, cells + [(i, j)], runs, 'M')
        if j < n:
            go(i, j + 1, start, cells, runs[:-1] + [runs[-1] + 1] if last == 'D' else runs + [1], 'D')
        if i < m:
            go(i + 1, j, start, cells, runs[:-1] + [runs[-1] + 1] if last == 'I' else runs + [1], 'I')
    for s in starts:
        go(s[0], s[1], s, [], [], None)
    return out


_PATHS = {}


def _shape(mode, m, n):
    """(paths, incidence of M cells as a P x (m n) matrix), built once per shape"""
    key = (mode, m, n)
    if key not in _PATHS:
        paths = _paths(mode, m, n)
        inc = np.zeros((len(paths), max(m * n, 1)), dtype=np.int64)
        for p, (_, _, cells, _) in enumerate(paths):
            for i, j in cells:
                inc[p, i * n + j] = 1
        _PATHS[key] = (paths, inc)
    return _PATHS[key]


def _best_per_end(mode, q, r, costs):
    """{end cell: the greatest score over all alignments that end there}, every maximal run costed by the cheaper piece"""
    m, n = len(q), len(r)
    paths, inc = _shape(mode, m, n)
    s = np.array([int(MAT[r[j]][q[i]]) for i in range(m) for j in range(n)] or [0], dtype=np.int64)
    gaps = np.array([sum(chk.gap(k, costs) for k in runs) for _, _, _, runs in paths], dtype=np.int64)
    scores = inc @ s - gaps
    best = {}
    for (_, end, _, _), v in zip(paths, scores):
        if end not in best or v > best[end]:
            best[end] = int(v)
    return best


def _end_by_rule(mode, m, n, best):
    """the end cell the tie rules pick among the cells' best scores"""
    if mode == 'global':
        return (m, n)
    if mode in ('semiglobal', 'prefix'):
        return max(((m, j) for j in range(n + 1)), key=lambda c: (best[c], -c[1]))
    if mode == 'overlap':
        cell = max(((m, j) for j in range(n + 1)), key=lambda c: (best[c], -c[1]))
        for i in range(m):
            if best[(i, n)] > best[cell]:
                cell = (i, n)
        return cell
    return max(best, key=lambda c: (best[c], -c[0], -c[1]))


@pytest.mark.parametrize('costs', SMALL_COSTS)
@pytest.mark.parametrize('mode', chk.MODES)
def test_the_checker_equals_the_enumeration_of_every_alignment_up_to_4_by_4(mode, costs):
    words = [chk.encode(w) for w in _small_words()]
    for q in words:
        for r in words:
            best = _best_per_end(mode, q, r, costs)
            end = _end_by_rule(mode, len(q), len(r), best)
            got = chk.plain(q, r, MAT, costs, mode)
            assert (got['score'], got['query_end'] + 1, got['ref_end'] + 1) == (best[end], end[0], end[1]), (q, r, got)
            chk.check_cigar(got, q, r, MAT, costs, mode)


def _seeded_pairs(tag, count, max_len, alphabet='ACGT'):
    rng = chk.rng_for('twopiece host', tag)
    out = []
    for t in range(count):
        r = chk.random_seq(rng, rng.randint(0 if t % 7 == 0 else 1, max_len), alphabet)
        q = chk.mutate(rng, r, 0.3, alphabet) if t % 3 else chk.random_seq(rng, rng.randint(0 if t % 5 == 0 else 1, max_len), alphabet)
        out.append((chk.encode(q), chk.encode(r)))
    return out


@pytest.mark.parametrize('costs', SMALL_COSTS + [(4, 2, 24, 1), (11, 1, 30, 0)])
def test_row_by_row_equals_cell_by_cell(costs):
    for q, r in _seeded_pairs('rows', 60, 40):
        for mode in chk.MODES:
            want = chk.plain(q, r, MAT, costs, mode)
            assert chk.align(q, r, MAT, costs, mode) == want
            assert chk.align(q, r, MAT, costs, mode, path=False)['score'] == want['score']
            chk.check_cigar(want, q, r, MAT, costs, mode)


@pytest.mark.parametrize('go,ge', [(3, 1), (4, 2), (2, 2), (8, 0)])
def test_a_dominated_second_piece_is_the_one_piece_checker_field_by_field(go, ge):
    for costs in ((go, ge, go, ge), (go, ge, go + 5, ge)):
        for q, r in _seeded_pairs('dominated', 40, 40):
            for mode in chk.MODES:
                one = (ec.align if mode in ec.MODES else ac.align)(q, r, MAT, go, ge, mode)
                assert chk.align(q, r, MAT, costs, mode) == one, (costs, mode)
                assert chk.plain(q, r, MAT, costs, mode) == one, (costs, mode)


def test_the_pieces_swap_where_the_costs_say():
    assert [chk.gap(k, (3, 2, 6, 1)) for k in (1, 4, 5, 6)] == [3, 9, 10, 11]           # equal at 4, piece 2 below from 5 on
    assert [chk.gap(k, (4, 2, 24, 1)) for k in (20, 21, 22)] == [42, 44, 45]            # piece 2 below from 22 on
    assert chk.violated((3, 2, 6, 1)) is None and chk.violated((2, 2, 2, 2)) is None and chk.violated((0, 0, 0, 0)) is None
    assert chk.violated((3, 2, 6, -1)) == '0 <= gap_extend2'
    assert chk.violated((3, 2, 6, 3)) == 'gap_extend2 <= gap_extend'
    assert chk.violated((1, 2, 6, 1)) == 'gap_extend <= gap_open'
    assert chk.violated((3, 2, 2, 1)) == 'gap_open <= gap_open2'


# ---- the scheme of the kernel against the definition ------------------------------------------------------------------------------
GEOMETRIES = [(1, 1), (1, 3), (3, 1), (8, 2)]          # (columns per lane, lanes): chunks of 1, 3, 3 and 16 columns


@pytest.mark.parametrize('cpl,lanes', GEOMETRIES)
@pytest.mark.parametrize('costs', SMALL_COSTS)
def test_the_scheme_of_the_kernel_equals_the_definition_on_every_small_pair(costs, cpl, lanes):
    """every pair over AC up to 4 x 4 (more than one chunk at most geometries): the scan of a piece never sees the other piece's E
    through H, and nothing the walk reads differs for it"""
    words = [chk.encode(w) for w in _small_words()]
    for q in words:
        for r in words:
            for mode in chk.MODES:
                assert mdl.run(q, r, MAT, costs, mode, cpl, lanes) == chk.plain(q, r, MAT, costs, mode), (q, r, mode)


@pytest.mark.parametrize('cpl,lanes', [(2, 3), (8, 2)])
def test_the_scheme_of_the_kernel_equals_the_definition_on_seeded_pairs(cpl, lanes):
    for costs in SMALL_COSTS + [(4, 2, 24, 1), (2, 1, 3, 1), (5, 5, 9, 5)]:
        for q, r in _seeded_pairs('scheme', 6, 30, 'AC' if costs[0] < 2 else 'ACGT'):
            if len(q) == 0 or len(r) == 0:
                continue
            for mode in chk.MODES:
                want = chk.align(q, r, MAT, costs, mode)
                assert mdl.run(q, r, MAT, costs, mode, cpl, lanes) == want, (costs, mode)
                assert mdl.run(q, r, MAT, costs, mode, cpl, lanes, store=False)['score'] == want['score']


def _long_gap_pairs():
    """a reference of 60 letters and copies that miss, or add, 12 letters: at (3, 2, 6, 1) a gap piece 2 pays for (17 against 25),
    placed so that it crosses the border between chunks of the small geometries"""
    rng = chk.rng_for('twopiece host', 'long gaps')
    ref = chk.random_seq(rng, 60)
    pairs = []
    for a in (10, 17, 26):
        pairs.append((ref[:a] + ref[a + 12:], ref))                      # 12 D
        pairs.append((ref[:a] + chk.random_seq(rng, 12, 'T') + ref[a:], ref))   # 12 I
    return [(chk.encode(q), chk.encode(r)) for q, r in pairs]


def _caught(fault, pairs, costs, modes=('global',), cpl=2, lanes=4):
    """the number of (pair, mode) at which the model with `fault` planted differs from the definition; without it, none"""
    bad = 0
    for q, r in pairs:
        for mode in modes:
            want = chk.align(q, r, MAT, costs, mode)
            assert mdl.run(q, r, MAT, costs, mode, cpl, lanes) == want
            try:
                bad += mdl.run(q, r, MAT, costs, mode, cpl, lanes, fault=fault) != want
            except (AssertionError, KeyError):
                bad += 1
    return bad


def test_planted_fault_piece_two_opened_at_go1_is_caught_by_the_long_gaps():
    assert _caught('open2_go1', _long_gap_pairs(), (3, 2, 6, 1)) > 0


def test_planted_fault_e2_dropped_from_the_hand_over_is_caught_by_gaps_across_a_chunk_border():
    # chunks of 8 columns: the 12-letter deletions cross a border in a piece-2 run
    assert _caught('handover_e2', _long_gap_pairs(), (3, 2, 6, 1)) > 0


def test_planted_fault_e2_opened_bit_read_from_piece_one_is_caught_by_the_long_deletions():
    assert _caught('bit_e2', _long_gap_pairs(), (3, 2, 6, 1)) > 0


def test_planted_fault_e2_preferred_on_a_tie_is_caught_where_piece_two_extends_for_free():
    # at ge2 = 0 an E_2 that opened further left keeps its value along the row and ties with an E_1 that opens here: the walk must
    # take E_1 and its shorter run, a CIGAR of the same score and another shape
    rng = chk.rng_for('twopiece host', 'tie')
    pairs = []
    for t in range(150):
        r = chk.random_seq(rng, rng.randint(6, 16), 'AC')
        q = chk.mutate(rng, r, 0.4, 'AC')
        if q:
            pairs.append((chk.encode(q), chk.encode(r)))
    assert _caught('e2_first', pairs, (2, 1, 3, 0), modes=('global', 'semiglobal')) > 0


def test_planted_fault_boundary_gap_costed_by_piece_one_alone_is_caught_by_long_end_gaps():
    rng = chk.rng_for('twopiece host', 'boundary')
    ref = chk.random_seq(rng, 40)
    pairs = [(chk.encode(ref[15:]), chk.encode(ref)), (chk.encode(ref), chk.encode(ref[15:]))]      # 15 letters before (0, 0) can only be a boundary gap
    assert _caught('boundary1', pairs, (3, 2, 6, 1), modes=('global', 'prefix')) > 0


def test_every_planted_fault_changes_nothing_where_the_pieces_are_equal_or_gaps_are_short():
    """the case sets above are what catches the faults: on pairs without a long gap, or with equal pieces, most stay silent"""
    rng = chk.rng_for('twopiece host', 'silent')
    ref = chk.random_seq(rng, 30)
    pairs = [(chk.encode(ref[:12] + ref[13:]), chk.encode(ref))]
    assert _caught('open2_go1', pairs, (3, 2, 6, 1)) == 0
    assert _caught('boundary1', pairs, (3, 2, 6, 1)) == 0


# ---- the keywords ------------------------------------------------------------------------------------------------------------------
def test_one_keyword_without_the_other_is_a_value_error():
    from ciri_long_amd import hip, ssw_wrap
    with pytest.raises(ValueError, match='gap_open2 and gap_extend2 come together'):
        ssw_wrap.align_pairs_ends(['ACGT'], ['ACGT'], gap_open2=24)
    with pytest.raises(ValueError, match='gap_open2 and gap_extend2 come together'):
        ssw_wrap.align_pairs_ends(['ACGT'], ['ACGT'], gap_extend2=1)
    with pytest.raises(ValueError, match='gap_open2 and gap_extend2 come together'):
        ssw_wrap.extend_anchors(['ACGT'], ['ACGT'], [(0, 0)], gap_open2=24)
    with pytest.raises(ValueError, match='gap_open2 and gap_extend2 come together'):
        hip.gap2_of('x', None, 1)
    with pytest.raises(ValueError, match='gap_open2 and gap_extend2 come together'):
        ssw_wrap.align_pairs_band(['ACGT'], ['ACGT'], 8, gap_extend2=1)
    with pytest.raises(ValueError, match='gap_open2 and gap_extend2 come together'):
        ssw_wrap.extend_anchors(['ACGT'], ['ACGT'], [(0, 0)], band=8, gap_open2=24)
    assert hip.gap2_of('x', None, None) is None
    g = hip.gap2_of('x', 24, 1)
    assert (g.gap_open2, g.gap_extend2) == (24, 1)


def test_the_long_read_preset_is_admitted_and_its_pieces_swap_at_22_letters():
    from ciri_long_amd import ssw_wrap
    p = ssw_wrap.LONG_READ_GAPS
    assert p == dict(match=2, mismatch=4, gap_open=4, gap_extend=2, gap_open2=24, gap_extend2=1)
    costs = (p['gap_open'], p['gap_extend'], p['gap_open2'], p['gap_extend2'])
    assert chk.violated(costs) is None
    assert min(k for k in range(1, 100) if costs[2] + (k - 1) * costs[3] < costs[0] + (k - 1) * costs[1]) == 22


# ---- the band ------------------------------------------------------------------------------------------------------------------------
def _bands(mode, m, n):
    """every clipped band [lo, hi] of an m x n pair that the mode admits"""
    return [(lo, hi) for lo in range(-m, n + 1) for hi in range(lo, n + 1) if chk.refusal(mode, m, n, lo, hi) is None]


def _band_best_per_end(mode, q, r, costs, lo, hi):
    """_best_per_end over the alignments all of whose cells lie in the band"""
    m, n = len(q), len(r)
    paths, inc = _shape(mode, m, n)
    s = np.array([int(MAT[r[j]][q[i]]) for i in range(m) for j in range(n)] or [0], dtype=np.int64)
    gaps = np.array([sum(chk.gap(k, costs) for k in runs) for _, _, _, runs in paths], dtype=np.int64)
    scores = inc @ s - gaps
    best = {}
    for (start, end, cells, runs), v, (dlo, dhi) in zip(paths, scores, _diag_spans(mode, m, n)):
        if lo <= dlo and dhi <= hi and (end not in best or v > best[end]):
            best[end] = int(v)
    return best


_SPANS = {}


def _diag_spans(mode, m, n):
    """(smallest, greatest) diagonal j - i over the cells of every path of _shape(mode, m, n), in its order"""
    key = (mode, m, n)
    if key not in _SPANS:
        out = []

        def go(i, j, dlo, dhi):
            d = j - i
            dlo, dhi = min(dlo, d), max(dhi, d)
            if _is_end(mode, m, n, i, j):
                out.append((dlo, dhi))
            if i < m and j < n:
                go(i + 1, j + 1, dlo, dhi)
            if j < n:
                go(i, j + 1, dlo, dhi)
            if i < m:
                go(i + 1, j, dlo, dhi)
        if mode in ('global', 'prefix', 'extend'):
            starts = [(0, 0)]
        else:
            starts = [(0, j) for j in range(n + 1)]
        for si, sj in starts:
            go(si, sj, sj - si, sj - si)
        assert len(out) == len(_shape(mode, m, n)[0])
        _SPANS[key] = out
    return _SPANS[key]


def _is_end(mode, m, n, i, j):
    if mode == 'global':
        return (i, j) == (m, n)
    if mode in ('semiglobal', 'prefix'):
        return i == m
    return True


def _band_end_by_rule(mode, m, n, best):
    if mode == 'global':
        return (m, n)
    if mode in ('semiglobal', 'prefix'):
        return max((c for c in best if c[0] == m), key=lambda c: (best[c], -c[1]))
    return max(best, key=lambda c: (best[c], -c[0], -c[1]))


@pytest.mark.parametrize('costs', SMALL_COSTS)
@pytest.mark.parametrize('mode', chk.BAND_MODES)
def test_the_banded_checker_equals_the_enumeration_inside_every_admitted_band(mode, costs):
    """every admitted band of every pair over AC up to 4 x 4 (the recursion of _diag_spans visits the paths in the order of _paths)"""
    words = [chk.encode(w) for w in _small_words()]
    count = 0
    for q in words:
        for r in words:
            for lo, hi in _bands(mode, len(q), len(r)):
                best = _band_best_per_end(mode, q, r, costs, lo, hi)
                end = _band_end_by_rule(mode, len(q), len(r), best)
                got = chk.plain_band(q, r, MAT, costs, mode, lo, hi)
                assert (got['score'], got['query_end'] + 1, got['ref_end'] + 1) == (best[end], end[0], end[1]), (q, r, lo, hi, got)
                chk.check_cigar(got, q, r, MAT, costs, mode)
                count += 1
    assert count > 10000


@pytest.mark.parametrize('costs', [(3, 2, 6, 1), (1, 1, 3, 0), (4, 2, 24, 1)])
def test_banded_row_by_row_equals_cell_by_cell_and_the_whole_band_is_the_full_matrix(costs):
    rng = chk.rng_for('twopiece host', 'band rows', costs)
    for q, r in _seeded_pairs(('band rows', costs), 50, 36):
        m, n = len(q), len(r)
        if not m or not n:
            continue
        for mode in chk.BAND_MODES:
            lo, hi = chk.band_of(mode, m, n, rng.randint(0, 10), None if rng.random() < 0.5 else rng.randint(-6, 6))
            if lo > hi or chk.refusal(mode, m, n, lo, hi) is not None:
                continue
            want = chk.plain_band(q, r, MAT, costs, mode, lo, hi)
            assert chk.align_band(q, r, MAT, costs, mode, lo, hi) == want
            chk.check_cigar(want, q, r, MAT, costs, mode)
            whole = chk.align_band(q, r, MAT, costs, mode, -m, n)
            assert whole['exact'] == 1 and chk.as_tuple(whole) == chk.as_tuple(chk.align(q, r, MAT, costs, mode))


@pytest.mark.parametrize('go,ge', [(3, 1), (4, 2)])
def test_a_dominated_second_piece_is_the_one_piece_banded_checker_field_by_field(go, ge):
    import band_check as bc
    rng = chk.rng_for('twopiece host', 'band dominated', go, ge)
    for costs in ((go, ge, go, ge), (go, ge, go + 5, ge)):
        for q, r in _seeded_pairs('band dominated', 40, 36):
            m, n = len(q), len(r)
            if not m or not n:
                continue
            for mode in chk.BAND_MODES:
                lo, hi = chk.band_of(mode, m, n, rng.randint(0, 9))
                if chk.refusal(mode, m, n, lo, hi) is not None:
                    continue
                one = (bc.align if mode in bc.MODES else ac.align_band)(q, r, MAT, go, ge, mode, lo, hi)
                assert chk.align_band(q, r, MAT, costs, mode, lo, hi) == one, (costs, mode)      # 'band' and 'exact' included


def _exact_pairs():
    """3 000 seeded pairs with an admitted band (draws whose band is refused are passed over), of up to 40 letters under half-widths
    0..12: copies with scattered edits, with one planted deletion or insertion of 3..12 letters (at (3, 2, 6, 1) the pieces swap at
    5), and unrelated sequences"""
    rng = chk.rng_for('twopiece host', 'exact', 1)
    made = 0
    for t in itertools.count():
        if made == 3000:
            return
        mode = ('global', 'prefix', 'extend')[t % 3]
        n = rng.randint(1, 40)
        r = chk.random_seq(rng, n)
        kind = t % 4
        if kind == 0:
            q = chk.mutate(rng, r, 0.15)
        elif kind == 1:
            a = rng.randint(0, n); L = rng.randint(3, 12); q = chk.mutate(rng, r[:a] + r[a + L:], 0.05)
        elif kind == 2:
            a = rng.randint(0, n); L = rng.randint(3, 12); q = chk.mutate(rng, r[:a] + chk.random_seq(rng, L) + r[a:], 0.05)
        else:
            q = chk.random_seq(rng, rng.randint(1, 40))
        q = q[:40] or 'A'
        w = rng.randint(0, 12)
        lo, hi = chk.band_of(mode, len(q), n, w)
        if chk.refusal(mode, len(q), n, lo, hi) is None:
            made += 1
            yield mode, chk.encode(q), chk.encode(r), lo, hi


def test_no_exact_certificate_is_wrong_and_exact_from_piece_one_alone_would_be():
    """`exact` over 3 000 seeded pairs at (3, 2, 6, 1): every certified row is the unbanded row; the counts of certified, equal
    without a certificate and different pairs are those recorded in DESIGN.md section 6; the certificate computed with piece 1
    alone (a planted fault: g too large for long runs) certifies rows that differ"""
    costs = (3, 2, 6, 1)
    counts = {'certified': 0, 'equal': 0, 'different': 0}
    wrong_with_piece_one = 0
    for mode, q, r, lo, hi in _exact_pairs():
        banded = chk.align_band(q, r, MAT, costs, mode, lo, hi)
        same = chk.as_tuple(banded) == chk.as_tuple(chk.align(q, r, MAT, costs, mode))
        if banded['exact']:
            assert same, (mode, q, r, lo, hi)
            counts['certified'] += 1
        else:
            counts['equal' if same else 'different'] += 1
        faulty = chk.exact_flag(mode, len(q), len(r), lo, hi, banded['score'], MAT, (costs[0], costs[1], costs[0], costs[1]))
        wrong_with_piece_one += bool(faulty and not same)
    assert counts == {'certified': 2049, 'equal': 573, 'different': 378}
    assert wrong_with_piece_one == 8


def test_semiglobal_rows_are_certified_only_when_the_band_is_the_whole_matrix():
    costs = (3, 2, 6, 1)
    rng = chk.rng_for('twopiece host', 'exact semiglobal')
    for q, r in _seeded_pairs('exact semiglobal', 40, 30):
        m, n = len(q), len(r)
        if not m or not n:
            continue
        lo, hi = chk.band_of('semiglobal', m, n, rng.randint(0, 12))
        if chk.refusal('semiglobal', m, n, lo, hi) is None:
            assert chk.align_band(q, r, MAT, costs, 'semiglobal', lo, hi)['exact'] == int(lo <= -m and hi >= n)
        whole = chk.align_band(q, r, MAT, costs, 'semiglobal', -m, n)
        assert whole['exact'] == 1 and chk.as_tuple(whole) == chk.as_tuple(chk.align(q, r, MAT, costs, 'semiglobal'))


# ---- the scheme of the banded kernel against the definition ----------------------------------------------------------------------
BAND_GEOMETRIES = [(1, 9), (2, 5), (3, 3)]             # (positions per lane, lanes): every band of a pair up to 4 x 4 fits (9 diagonals)


@pytest.mark.parametrize('cpl,lanes', BAND_GEOMETRIES)
@pytest.mark.parametrize('costs', SMALL_COSTS)
def test_the_scheme_of_the_banded_kernel_equals_the_definition_on_every_small_pair_and_band(costs, cpl, lanes):
    """every pair over AC up to 4 x 4, every mode, every admitted band: the two scans in the band's frame, their minus infinity and
    the missing cross term change nothing the definition says, field by field with `exact`"""
    words = [chk.encode(w) for w in _small_words()]
    count = 0
    for q in words:
        for r in words:
            for mode in chk.BAND_MODES:
                for lo, hi in _bands(mode, len(q), len(r)):
                    assert mdl.run_band(q, r, MAT, costs, mode, lo, hi, cpl, lanes) == chk.plain_band(q, r, MAT, costs, mode, lo, hi), (q, r, mode, lo, hi)
                    count += 1
    assert count > 40000


def _with_band(pairs, w, modes, costs, width=32):
    out = []
    for q, r in pairs:
        for mode in modes:
            if len(q) and len(r):
                lo, hi = chk.band_of(mode, len(q), len(r), w)
                if chk.refusal(mode, len(q), len(r), lo, hi) is None and hi - lo + 1 <= width:
                    out.append((q, r, mode, lo, hi, costs))
    return out


@pytest.mark.parametrize('cpl,lanes', [(2, 16), (8, 4), (4, 64)])
def test_the_scheme_of_the_banded_kernel_equals_the_definition_on_seeded_pairs(cpl, lanes):
    for costs in SMALL_COSTS + [(4, 2, 24, 1), (5, 5, 9, 5)]:
        for w in (2, 9):
            for q, r, mode, lo, hi, _ in _with_band(_seeded_pairs('band scheme', 8, 30), w, chk.BAND_MODES, costs):
                want = chk.align_band(q, r, MAT, costs, mode, lo, hi)
                assert mdl.run_band(q, r, MAT, costs, mode, lo, hi, cpl, lanes) == want, (costs, mode, lo, hi)
                assert mdl.run_band(q, r, MAT, costs, mode, lo, hi, cpl, lanes, store=False)['score'] == want['score']


def _band_sets():
    costs = (3, 2, 6, 1)
    rng = chk.rng_for('twopiece host', 'band tie')
    tie = []
    for t in range(150):
        r = chk.random_seq(rng, rng.randint(6, 16), 'AC')
        q = chk.mutate(rng, r, 0.4, 'AC')
        if q:
            tie.append((chk.encode(q), chk.encode(r)))
    rng = chk.rng_for('twopiece host', 'boundary')
    ref = chk.random_seq(rng, 40)
    ends = [(chk.encode(ref[15:]), chk.encode(ref)), (chk.encode(ref), chk.encode(ref[15:]))]
    return {'long gaps': _with_band(_long_gap_pairs(), 14, ('global', 'extend'), costs),
            'free piece-2 ties': _with_band(tie, 5, ('global', 'semiglobal'), (2, 1, 3, 0)),
            'long end gaps': _with_band(ends, 3, ('global',), costs),
            'random': _with_band(_seeded_pairs('band faults', 30, 24), 4, chk.BAND_MODES, costs)}


BAND_FAULT_SETS = [('open2_go1', 'long gaps'), ('bit_e2', 'long gaps'), ('e2_first', 'free piece-2 ties'), ('boundary1', 'long end gaps'),
                   ('f2_own', 'random'), ('f2_own', 'long gaps'), ('e2_seed', 'random'), ('exact1', 'random')]


@pytest.mark.parametrize('fault,name', BAND_FAULT_SETS)
def test_a_planted_fault_in_the_banded_model_is_caught_by_a_named_set(fault, name):
    bad = 0
    for q, r, mode, lo, hi, costs in _band_sets()[name]:
        want = chk.align_band(q, r, MAT, costs, mode, lo, hi)
        assert mdl.run_band(q, r, MAT, costs, mode, lo, hi, 2, 16) == want               # the model as it stands passes the set
        try:
            bad += mdl.run_band(q, r, MAT, costs, mode, lo, hi, 2, 16, fault=fault) != want
        except (AssertionError, KeyError):
            bad += 1
    assert bad > 0, (fault, name)


def test_admission_bound_of_the_banded_model_keeps_minus_infinity_apart_under_four_costs():
    """the largest cost the 2^29 bound admits for a 6 x 7 pair, in every seat of the four: every value the model meets passes its
    range checks (scores inside (-2^29, 2^29), what derives from minus infinity inside [-2^30 - 2^29, -2^30 + 2^29))"""
    m, n = 6, 7
    big = ((1 << 29) - 1) // (m + n + 2 * mdl.MAX_WIDTH)
    assert mdl.band_admitted(m, n, big) and not mdl.band_admitted(m, n, big + 1)
    rng = chk.rng_for('twopiece host', 'bound')
    q, r = chk.encode(chk.random_seq(rng, m)), chk.encode(chk.random_seq(rng, n))
    mat = chk.dna_matrix(127, 127)
    for costs in ((big, big, big, big), (big, 0, big, 0), (4, 2, big, 1), (big, big, big, 0), (0, 0, big, 0)):
        for mode in chk.BAND_MODES:
            lo, hi = chk.band_of(mode, m, n, 2)
            got = mdl.run_band(q, r, mat, costs, mode, lo, hi, cpl=8, lanes=64)
            assert got == chk.align_band(q, r, mat, costs, mode, lo, hi), (costs, mode)
