"""edlib.align on the GPU (K4m / K4t, csrc/edit_align.hip) at the edges tests/edlib_edges.py builds: every lane-group class with and
without idle lanes, two to four passes, reverse-pass slots beyond one launch, equalities over eight planes, the 8 / 9 letter
switch, the feeder at short targets, the k bound, workspace chunks and a plan run twice.  Every result is `==` the dict of
tests/edlib_check.py (the plain dynamic programme) and goes through check_invariants and check_locations, except two that the
full checker cannot afford:
  * the homopolymer pair (4097 x 22000) of test_reverse_launches: about 17 900 locations, each held to the family's closed form
    (edlib_edges.homopolymer_closed_form, which tests/test_edlib_edges_host.py holds to the checker on small members);
  * test_path_8193_three_passes: locations and distance `==` the checker's, the CIGAR through check_invariants (valid, of exactly
    the optimal cost, over exactly target[start..end]) -- the checker's own CIGAR would need the whole 8193 x 8400 matrix."""
import pytest

import edlib_check
import edlib_edges as E

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    from ciri_long_amd import hip
    c = hip.Context(0)
    yield c
    c.close()


_proved = {}


def _run(ctx, b, k=None):
    from ciri_long_amd import edlib
    return edlib.align_batch(b.queries, b.targets, b.mode, b.task, b.k if k is None else k, b.equalities, ctx, b.workspace_bytes)


def _check(b, got, k=None, skip=()):
    """every result equal to the checker's dict, then the invariants -> the number of locations whose start was proved"""
    assert len(got) == len(b.queries)
    proved = 0
    for i, (q, t, g) in enumerate(zip(b.queries, b.targets, got)):
        if i in skip:
            continue
        want = E.expected(edlib_check, q, t, b.mode, b.task, b.k if k is None else k, b.equalities)
        assert g == want, (b.mode, b.task, i, len(q), len(t), q[:60], t[:60], str(g)[:300], str(want)[:300])
        edlib_check.check_invariants(g, q, t, b.mode, b.equalities)
        key = (q, t, b.mode, tuple(b.equalities or ()), tuple(g['locations']))     # the same locations are proved once
        if key not in _proved:
            _proved[key] = edlib_check.check_locations(g, q, t, b.mode, b.equalities, seed=i)
        proved += _proved[key]
    return proved


@pytest.mark.parametrize('alpha', ['dna', 'aa20'])
@pytest.mark.parametrize('mode', E.MODES)
@pytest.mark.parametrize('task', E.TASKS)
def test_classes(ctx, alpha, mode, task):
    b, = [b for b in E.classes()[(0 if alpha == 'dna' else 9):][:9] if (b.mode, b.task) == (mode, task)]
    proved = _check(b, _run(ctx, b))
    assert task == 'distance' or proved >= len(b.queries)


@pytest.mark.parametrize('mode', E.MODES)
def test_passes_short_targets(ctx, mode):
    b, = [b for b in E.passes_short() if b.mode == mode]
    assert _check(b, _run(ctx, b)) >= len(b.queries)


@pytest.mark.parametrize('mode', E.MODES)
def test_passes_long_targets(ctx, mode):
    b, = [b for b in E.passes_long() if b.mode == mode]
    assert _check(b, _run(ctx, b)) >= len(b.queries)


def test_path_8193_three_passes(ctx):
    b = E.pass_path_8193()
    g, = _run(ctx, b)
    q, t = b.queries[0], b.targets[0]
    assert dict(g, cigar=None) == E.expected(edlib_check, q, t, 'HW', 'locations')
    assert g['cigar'] is not None
    edlib_check.check_invariants(g, q, t, 'HW')
    assert edlib_check.check_locations(g, q, t, 'HW') > 0


def test_reverse_launches(ctx):
    b, long_i, hom_i, mid_i = E.reverse_launches()
    got = _run(ctx, b)
    m, n, x = E.REVERSE_HOMOPOLYMER
    want = E.homopolymer_closed_form(m, n, x)
    g = got[hom_i]
    print('homopolymer pair: distance', g['editDistance'], 'locations', len(g['locations']), 'want', len(want['locations']))
    assert g['editDistance'] == want['editDistance'] and g['alphabetLength'] == want['alphabetLength'] and g['cigar'] is None
    assert len(g['locations']) == n - m + x + 1
    bad = [(i, a, w) for i, (a, w) in enumerate(zip(g['locations'], want['locations'])) if a != w]
    assert not bad, (len(bad), bad[:5], bad[-5:])
    assert _check(b, got, skip=(hom_i,)) >= len(b.queries) - 1


@pytest.mark.parametrize('name', ['eq_protein', 'eq_bytes', 'eq_bytes_absent', 'eq_iupac'])
@pytest.mark.parametrize('mode', E.MODES)
def test_equalities_over_eight_planes(ctx, name, mode):
    b, = [b for b in getattr(E, name)() if b.mode == mode]
    got = _run(ctx, b)
    assert _check(b, got) >= len(b.queries)
    if name == 'eq_iupac':          # N = A and N = C do not make A = C (HW ends before the target first: 1I)
        assert (b.queries[-1], b.targets[-1]) == (b'A', b'C') and got[-1]['editDistance'] == 1
        assert got[-1]['cigar'] == ('1I' if mode == 'HW' else '1X')


def test_eight_and_nine_letters(ctx):
    """the planes are chosen per batch (3 up to 8 letters, else 8): a pair's answer does not depend on the batch it travels in"""
    from ciri_long_amd import edlib
    for b8, b9 in E.eight_and_nine():
        got8, got9 = _run(ctx, b8), _run(ctx, b9)
        assert got9[:len(got8)] == got8
        alone = [edlib.align(q, t, b9.mode, b9.task, b9.k, b9.equalities) for q, t in zip(b9.queries, b9.targets)]
        assert alone == got9
        assert _check(b9, got9) >= len(b9.queries)


@pytest.mark.parametrize('mode', E.MODES)
def test_feeder(ctx, mode):
    for b in E.feeder():
        if b.mode == mode:
            assert _check(b, _run(ctx, b)) >= len(b.queries)


@pytest.mark.parametrize('mode', E.MODES)
def test_k(ctx, mode):
    """k = d keeps the free result, k = d - 1 leaves the empty one, k = 0 only an identical pair, k above m everything; d is the
    checker's"""
    empties = kept = 0
    for b, d in E.k_batches(edlib_check, (mode,)):
        got = _run(ctx, b)
        _check(b, got)
        assert (got[0]['editDistance'] == -1) == (d > b.k)
        empties += d > b.k; kept += d <= b.k
    assert empties > 50 and kept > 50
    q, t, _ = E.k_pairs()[-1]
    assert q == t and _run(ctx, E.Batch([q], [t], mode, 'path', 0, None, 0))[0]['cigar'] == '%d=' % len(q)


def test_workspace_chunks_and_the_exact_limit(ctx):
    from ciri_long_amd import hip
    ws, one = E.all_cases()['workspace']
    assert len(E.workspace_chunks(ws)) >= 3
    assert _check(ws, _run(ctx, ws)) >= len(ws.queries)
    assert _check(one, _run(ctx, one)) == 1                                     # workspace_bytes == the pair's bytes: runs
    with pytest.raises(hip.ClhError, match='workspace'):
        _run(ctx, one._replace(workspace_bytes=one.workspace_bytes - 1))


def test_plan_runs_twice(ctx):
    """a plan keeps its device buffers (ends, reverse results, carries, workspace): the second run sees none of the first"""
    from ciri_long_amd import edlib
    b = E.plan_batch()
    plan = ctx.edit_align_plan(b.queries, b.targets, b.mode, b.task)
    try:
        for _ in range(2):
            plan.run()
            _check(b, edlib.results_from_rows(*plan.fetch(), task=b.task))
    finally:
        plan.close()
