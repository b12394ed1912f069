"""CPU statements to tests/edlib_edges.py: tools/edit_align_model.py (the block and pass recurrences of K4m / K4t) against
tests/edlib_check.py (the plain dynamic programme) on the edge sets, the closed form of the homopolymer family against the checker,
and the proof that every set reaches what it is named for, from the plan's routing as edlib_edges restates it.

The model is pure Python (big integers, one block at a time), so it is thinned by length only, never by mode or task: it runs the
class set up to MODEL_CLASS_MAX letters (left out: 1024, 1025, 2048, 2049, 2113, 4095, 4096 -- the model knows blocks and passes, not
lanes, and a block count above 10 adds nothing to it), the equalities sets up to MODEL_EQ_MAX (left out: 2500 and 4200), the k set's
class pairs up to MODEL_CLASS_MAX, and of the pass set's short-target half every length (12289 included)."""
import os
import random
import sys

import pytest

import edlib_check
import edlib_edges as E

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
import edit_align_model as model  # noqa: E402

MODEL_CLASS_MAX = 577
MODEL_EQ_MAX = 1000


_proved = {}


def _model_batch(b, max_m, k=None):
    ran = 0
    for q, t in zip(b.queries, b.targets):
        if len(q) > max_m:
            continue
        want = E.expected(edlib_check, q, t, b.mode, b.task, b.k if k is None else k, b.equalities)
        got = model.align(q, t, b.mode, b.task, b.k if k is None else k, eq=b.equalities or ())
        assert got == want, (b.mode, b.task, len(q), len(t), q[:40], t[:40])
        edlib_check.check_invariants(got, q, t, b.mode, b.equalities)
        key = (q, t, b.mode, tuple(b.equalities or ()), tuple(got['locations']))     # the same locations are proved once
        if key not in _proved:
            _proved[key] = edlib_check.check_locations(got, q, t, b.mode, b.equalities)
        assert _proved[key] > 0 or not got['locations'] or got['locations'][0][0] is None
        ran += 1
    return ran


def test_expected_is_the_checker():
    """edlib_edges.expected derives 'locations', 'distance' and the k rule from one run of the checker: the same dicts as asking it"""
    rng = random.Random(5)
    for it in range(60):
        q, t = E.planted(rng, rng.randint(1, 90), E.DNA, 0.2, 40) if it % 2 else E.tandem(rng, rng.randint(2, 90), E.DNA)
        for mode in E.MODES:
            d = edlib_check.align(q, t, mode)['editDistance']
            for task in rng.sample(E.TASKS, 3):
                for k in (-1, d, d - 1, 0, len(q) + 1):
                    assert E.expected(edlib_check, q, t, mode, task, k) == edlib_check.align(q, t, mode, task, k), (q, t, mode, task, k)


@pytest.mark.parametrize('alpha', ['dna', 'aa20'])
@pytest.mark.parametrize('mode', E.MODES)
@pytest.mark.parametrize('task', E.TASKS)
def test_model_on_the_classes(alpha, mode, task):
    b, = [b for b in E.classes()[(0 if alpha == 'dna' else 9):][:9] if (b.mode, b.task) == (mode, task)]
    assert E.letters(b) == (4 if alpha == 'dna' else 20)
    assert _model_batch(b, MODEL_CLASS_MAX) >= 27 + 4


@pytest.mark.parametrize('mode', E.MODES)
def test_model_on_the_short_target_passes(mode):
    b, = [b for b in E.passes_short() if b.mode == mode]
    assert _model_batch(b, 1 << 30) == 2 * len(E.PASS_LENGTHS)


@pytest.mark.parametrize('name', ['eq_protein', 'eq_bytes', 'eq_bytes_absent', 'eq_iupac'])
def test_model_on_equalities_over_eight_planes(name):
    for b in getattr(E, name)():
        assert _model_batch(b, MODEL_EQ_MAX) >= 3
    if name == 'eq_iupac':
        b = E.eq_iupac()[0]
        assert (b.queries[-1], b.targets[-1]) == (b'A', b'C')
        for mode in E.MODES:
            r = edlib_check.align(b'A', b'C', mode, 'path', -1, b.equalities)       # N = A, N = C, and A is not C
            assert r['editDistance'] == 1 and r['cigar'] == ('1I' if mode == 'HW' else '1X')      # HW: the end before the target comes first


def test_model_on_eight_and_nine_letters():
    for b8, b9 in E.eight_and_nine():
        assert _model_batch(b9, 1 << 30) == len(b9.queries)
        # the checker has no batch: the first N answers of both batches are the same calls
        assert b9.queries[:-1] == b8.queries and b9.targets[:-1] == b8.targets


def test_model_on_the_feeder():
    for b in E.feeder():
        assert _model_batch(b, 1 << 30) == len(E.FEEDER_M)


@pytest.mark.parametrize('mode', E.MODES)
def test_model_on_k(mode):
    ran = 0
    for b, d in E.k_batches(edlib_check, (mode,)):
        if len(b.queries[0]) > MODEL_CLASS_MAX and len(b.targets[0]) > 400:
            continue
        ran += _model_batch(b, 1 << 30)
    assert ran > 100


def test_banded_distance_is_the_distance():
    """edlib_check.nw_distance with a band w: the plain last-row distance when it is <= w, else w + 1"""
    rng = random.Random(17)
    eqm = edlib_check.eq_matrix()
    for it in range(300):
        q, t = E.planted(rng, rng.randint(1, 80), E.DNA, 0.2, 10) if it % 2 else E.unrelated(rng, rng.randint(1, 80), E.DNA)
        q, t = edlib_check._arr(q), edlib_check._arr(t)
        f = int(edlib_check.last_row(q, t, 'NW', eqm)[-1])
        for w in (0, 1, 3, 10, 40, 200):
            assert edlib_check.nw_distance(q, t, eqm, w) == (f if f <= w else w + 1), (it, w, f)


def test_homopolymer_closed_form():
    """the licence to hold the 4097 x 22000 pair of the reverse-launch set to the closed form: it is the checker's answer on
    400 random small members of the family, x = 0 among them"""
    rng = random.Random(31)
    for it in range(400):
        m = rng.randint(1, 40)
        x = 0 if it % 8 == 0 else rng.randint(0, min(m, 4))
        q, t = E.homopolymer(rng, m, rng.randint(m, 120), x)
        assert edlib_check.align(q, t, 'HW', 'locations') == E.homopolymer_closed_form(m, len(t), x), (q, len(t))


def test_check_locations_can_fail():
    """the location statement rejects a start that is not the smallest, and one whose slice has another distance"""
    q, t = b'ACGT', b'TTACGTACGTTT'
    good = edlib_check.align(q, t, 'HW', 'locations')
    assert good['locations'] == [(2, 5), (6, 9)] and edlib_check.check_locations(good, q, t, 'HW') == 2
    with pytest.raises(AssertionError):
        edlib_check.check_locations(dict(good, locations=[(3, 5), (6, 9)]), q, t, 'HW')
    hom = edlib_check.align(b'AACA', b'AAAAAA', 'HW', 'locations')          # the longest alignment: (0, 3), though AAA at 1..3 costs 1 too
    assert hom['locations'][:2] == [(0, 2), (0, 3)] and edlib_check.check_locations(hom, b'AACA', b'AAAAAA', 'HW') == len(hom['locations'])
    with pytest.raises(AssertionError, match='smaller start'):
        edlib_check.check_locations(dict(hom, locations=[(0, 2), (1, 3)] + hom['locations'][2:]), b'AACA', b'AAAAAA', 'HW')
    # above 2**12 cells (the stepping forward search) and above 2**22 (sampled locations): a start one too large, a slice of another cost
    for m, n in ((100, 300), (2200, 2300)):
        q, t = E.homopolymer(random.Random(m), m, n, 2)
        hom = E.homopolymer_closed_form(m, n, 2)
        assert hom == edlib_check.align(q, t, 'HW', 'locations')
        if m > 100:
            hom = dict(hom, locations=hom['locations'][-6:])           # six locations: the first, the last and two others are searched
        assert edlib_check.check_locations(hom, q, t, 'HW') == (len(hom['locations']) if m == 100 else 4)
        last = len(hom['locations']) - 1
        s, e = hom['locations'][last]
        with pytest.raises(AssertionError, match='smaller start'):
            edlib_check.check_locations(dict(hom, locations=hom['locations'][:last] + [(s + 1, e)]), q, t, 'HW')
        with pytest.raises(AssertionError):
            edlib_check.check_locations(dict(hom, locations=hom['locations'][:last] + [(s - 3, e)]), q, t, 'HW')


def test_the_edges_are_reached():
    cases = E.all_cases()
    # 1. every lane-group class, and a group with idle lanes for every G >= 4; both alphabets; one batch per (mode, task)
    for alpha_batches, nletters in ((cases['classes'][:9], 4), (cases['classes'][9:], 20)):
        assert sorted((b.mode, b.task) for b in alpha_batches) == sorted((mo, ta) for mo in E.MODES for ta in E.TASKS)
        for b in alpha_batches:
            ms = [len(q) for q, t in zip(b.queries, b.targets) if q and t]
            assert sorted(set(ms)) == list(E.CLASS_LENGTHS) and all(ms.count(m) == 3 for m in E.CLASS_LENGTHS)
            assert {E.ea_group(m) for m in ms} == {1, 2, 4, 8, 16, 32, 64}
            for G in (4, 8, 16, 32, 64):
                assert any(E.ea_group(m) == G and E.idle_lanes(m) > 0 for m in ms), G
                assert any(E.ea_group(m) == G and E.idle_lanes(m) == 0 for m in ms), G
            assert (E.blocks(577), E.ea_group(577), E.blocks(2113), E.ea_group(2113)) == (10, 16, 34, 64)
            assert {E.passes(m) for m in ms} == {1} and 4096 in ms
            assert sum(not q for q in b.queries) == 3 and sum(not t for t in b.targets) == 3
            assert [E.ea_group(len(q)) for q in b.queries] != sorted(E.ea_group(len(q)) for q in b.queries)   # not in task order
            assert E.letters(b) == nletters
    # 2. passes
    for name in ('passes_short', 'passes_long'):
        assert sorted(b.mode for b in cases[name]) == sorted(E.MODES)
        for b in cases[name]:
            assert [E.passes(m) for m in sorted({len(q) for q in b.queries})] == [2, 2, 2, 3, 3, 4]
    assert E.blocks(8257) == 2 * 64 + 2 and E.blocks(8193) == 2 * 64 + 1 and E.blocks(12289) == 3 * 64 + 1
    assert all(1 <= len(t) <= 400 for t in cases['passes_short'][0].targets)
    assert sum(len(t) < 64 for t in cases['passes_short'][0].targets) == len(E.PASS_LENGTHS)         # shorter than the skew
    assert all(len(q) <= len(t) + 400 and len(t) <= len(q) + 1100 for q, t in zip(cases['passes_long'][0].queries, cases['passes_long'][0].targets))
    b = cases['passes_path_8193'][0]
    assert (b.mode, b.task, len(b.queries[0]), E.passes(8193)) == ('HW', 'path', 8193, 3) and len(b.targets[0]) > 8193
    # 3. reverse launches: one G = 64 class, both long pairs beyond one launch, a pair without carry buffers in it
    b, long_i, hom_i, mid_i = E.reverse_launches()
    assert (b.mode, b.task) == ('HW', 'locations')
    cls = [(len(q), len(t)) for q, t in zip(b.queries, b.targets) if E.ea_group(len(q)) == 64]
    slots = E.rev_launch_slots(cls)
    assert slots == (256 << 20) // (2 * E.ea_pad(max(min(n, 2 * m + 1) for m, n in cls if m > 4096))) and 15000 < slots < 16500
    assert len(cls) == 3 and sum(m > 4096 for m, _ in cls) == 2 and 2049 <= len(b.queries[mid_i]) <= 4096
    for i in (long_i, hom_i):
        assert len(b.queries[i]) > 4096 and len(b.targets[i]) + 1 > slots
    m, n, x = E.REVERSE_HOMOPOLYMER
    assert (len(b.queries[hom_i]), len(b.targets[hom_i]), b.queries[hom_i].count(b'C')) == (m, n, x) and 0 < x <= 5
    assert len(E.homopolymer_closed_form(m, n, x)['locations']) == n - m + x + 1 > slots       # the used slots straddle a launch border
    assert sum(n + 1 for _m, n in cls) > 2 * slots   # three launches
    # 4. equalities over eight planes
    for name, npartners in (('eq_protein', 23), ('eq_bytes', 255), ('eq_bytes_absent', 254), ('eq_iupac', 4)):
        assert sorted(b.mode for b in cases[name]) == sorted(E.MODES)
        for b in cases[name]:
            present = set(b''.join(b.queries)) | set(b''.join(b.targets))
            assert b.task == 'path' and len(present) > 8
            eq = b.equalities
            assert any(a in present and c in present and a != c for a, c in eq)
            partners = {}
            for a, c in eq:
                if a != c and a in present and c in present:
                    partners.setdefault(a, set()).add(c); partners.setdefault(c, set()).add(a)
            assert max(len(v) for v in partners.values()) >= npartners
            assert len(set(eq)) < len(eq)                                       # a duplicate
            assert any((c, a) in eq for a, c in eq if a != c)                   # a reversed duplicate
            assert any(a == c for a, c in eq)                                   # a self pair
            assert name == 'eq_bytes' or any(a not in present or c not in present for a, c in eq)
            assert {E.ea_group(len(q)) for q in b.queries} >= {1, 4, 16, 64} and max(E.passes(len(q)) for q in b.queries) == 2
    assert len(set(b''.join(cases['eq_bytes'][0].queries + cases['eq_bytes'][0].targets))) == 256
    absent = cases['eq_bytes_absent'][0]
    assert set(range(256)) - set(b''.join(absent.queries + absent.targets)) == {0xfe} and any(0xfe in p and max(p) > 127 and p[0] != p[1] for p in absent.equalities)
    assert len(set(b''.join(cases['eq_iupac'][0].queries + cases['eq_iupac'][0].targets))) == 15
    # 5. exactly 8 and 9 letters
    for b8, b9 in E.eight_and_nine():
        assert (E.letters(b8), E.letters(b9)) == (8, 9)
        assert {E.ea_group(len(q)) for q in b8.queries} >= {1, 2, 4, 8, 16, 32}
    # 6. the feeder
    assert len(cases['feeder']) == len(E.FEEDER_N) * 3
    for b in cases['feeder']:
        assert [len(q) for q in b.queries] == list(E.FEEDER_M) and len({len(t) for t in b.targets}) == 1
    assert sorted({len(b.targets[0]) for b in cases['feeder']}) == list(E.FEEDER_N)
    assert any(len(b.targets[-1]) < E.ea_group(len(b.queries[-1])) for b in cases['feeder'])
    # 8. workspace: at least three chunks of at least two classes each; the single pair's limit is its own bytes
    ws = cases['workspace'][0]
    chunks = E.workspace_chunks(ws)
    assert len(chunks) >= 3 and all(len({E.ea_group(m) for m, _ in ch}) >= 2 for ch in chunks), chunks
    assert all(E.path_bytes(m, n, ws.mode) <= ws.workspace_bytes for ch in chunks for m, n in ch)
    one = cases['workspace'][1]
    assert one.workspace_bytes == E.path_bytes(len(one.queries[0]), len(one.targets[0]), 'NW') == E.workspace()[2]
    assert one.workspace_bytes % 256 == 0 and len(E.workspace_chunks(one)) == 1
    # the plan case: every class and a second pass in one HW path batch
    pb = cases['plan'][0]
    assert {E.ea_group(len(q)) for q in pb.queries if q} == {1, 2, 4, 8, 16, 32, 64} and max(E.passes(len(q)) for q in pb.queries) == 2


def test_all_cases_are_the_builders():
    """all_cases() (what tests/golden/make_edlib_golden.py records) holds exactly the batches the two test modules take from the builders"""
    cases = E.all_cases()
    for name in ('classes', 'passes_short', 'passes_long', 'eq_protein', 'eq_bytes', 'eq_bytes_absent', 'eq_iupac', 'feeder'):
        assert cases[name] == getattr(E, name)()
    assert cases['passes_path_8193'] == [E.pass_path_8193()] and cases['reverse_launches'] == [E.reverse_launches()[0]]
    assert cases['eight_and_nine'] == [b9 for _, b9 in E.eight_and_nine()] and cases['plan'] == [E.plan_batch()]
    assert cases['k'] == [b for b, _ in E.k_batches(edlib_check)] and {b.k for b in cases['k']} > {0} and all(b.k >= 0 for b in cases['k'])
    assert cases['workspace'][0] == E.workspace()[0]
