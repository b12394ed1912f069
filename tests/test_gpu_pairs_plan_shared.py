"""What the two pair plans (K1g EndsPlan, K1gb BandPlan) share on the host -- the shares of the workspace, fetch and its CIGAR
capacity -- and the timed-run bracket all six plan kinds take from one place.  Expected rows are tests/band_check.py and
tests/ends_check.py; the capacity cases go through the C ABI itself (hip.lib()).  Sequences are a few hundred letters at most."""
import ctypes as C

import numpy as np
import pytest

import band_check as chk
import ends_check as ec
from test_gpu_band import _check, _class_of, _copy_of, _ctx, _dna, _rows, geom  # noqa: F401  (geom is a fixture)

pytestmark = pytest.mark.gpu

CLH_E_CAPACITY = -4         # include/ciri_long_hip.h
M = 70                      # query rows: past the 64-row reload of the letters


def _mixed_batch(mode, geom):
    """nine kernel pairs of M rows whose clipped widths fall in class 0, 2, 1, repeating in that order, a pair without a query letter
    behind the first and one without a reference letter behind the fourth -> (queries, references, half-width, diagonals or None)"""
    rng = chk.rng_for('gpu pairs plan shared', mode)
    cpl = geom['cpl']
    qs, rs, diags = [], [], []
    if mode == 'global':
        w = 32 * cpl[0] - 4                                      # equal lengths: 2 w + 1 diagonals, class 0; n - m more in a longer reference
        extra = {0: 0, 1: 64 * cpl[0], 2: 64 * cpl[1]}
        for k in range(9):
            r = chk.random_seq(rng, M + extra[(0, 2, 1)[k % 3]])
            rs.append(r); qs.append(_copy_of(rng, r, M)); diags.append(None)
        empty_q, empty_r = ('', chk.random_seq(rng, 5), None), (chk.random_seq(rng, 5), '', None)
    else:
        w = 20 * cpl[2]                                          # 2 w + 1 diagonals, class 2, where the matrix does not clip them
        assert 64 * cpl[1] < 2 * w + 1 <= 64 * cpl[2]
        n_of = {0: 40, 1: 150, 2: 2 * w + 1 + M + 9}             # [-m, n] clips the band to n + M + 1 diagonals in classes 0 and 1
        for k in range(9):
            c = (0, 2, 1)[k % 3]
            r = chk.random_seq(rng, n_of[c])
            d = w + 5 if c == 2 else min(30, n_of[c] // 2)
            rs.append(r); qs.append(_copy_of(rng, r[max(d, 0):], M)); diags.append(d)
        # without a query letter the row is the first cell of the band on row 0: column lo = 3
        empty_q, empty_r = ('', chk.random_seq(rng, 10), w + 3), (chk.random_seq(rng, 5), '', 0)
    for at, (q, r, d) in ((1, empty_q), (5, empty_r)):           # behind the first and behind the fourth kernel pair
        qs.insert(at, q); rs.insert(at, r); diags.insert(at, d)
    return qs, rs, w, (None if mode == 'global' else diags)


@pytest.mark.parametrize('mode', ['global', 'semiglobal'])
def test_shares_cut_through_classes_and_empty_sides_in_one_band_plan(geom, mode):
    qs, rs, w, diags = _mixed_batch(mode, geom)
    mat = chk.dna_matrix(10, 4)
    classes = []
    for k, (q, r) in enumerate(zip(qs, rs)):
        lo, hi = chk.band_of(len(q), len(r), w, None if diags is None else diags[k])
        assert chk.refusal(mode, len(q), len(r), lo, hi) is None
        classes.append(_class_of(geom, hi - lo + 1) if q and r else None)
    assert classes == [0, None, 2, 1, 0, None, 2, 1, 0, 2, 1]
    whole = {}
    one_share = _rows(_dna(qs), _dna(rs), mat, 8, 2, w, mode, diags, True, info=whole)
    assert whole['shares'] == 1 and whole['class_pairs'] == [3, 3, 3] and whole['empty_pairs'] == 2
    if mode == 'semiglobal':
        assert one_share[1][1:3] == (3, 2)                       # ref_begin = lo, ref_end = lo - 1
    cut = {}
    wants = _check(_dna(qs), _dna(rs), mat, 8, 2, w, mode, diagonals=diags, info=cut, workspace_bytes=whole['max_pair_bytes'])
    assert cut['shares'] > 1 and all(c > 0 for c in cut['class_pairs']) and cut['workspace_bytes'] <= whole['max_pair_bytes']
    assert one_share == [chk.as_tuple(x) for x in wants]
    more = {}
    got = _rows(_dna(qs), _dna(rs), mat, 8, 2, w, mode, diags, True, workspace_bytes=whole['max_pair_bytes'] + 16, info=more)
    assert more['shares'] > 1 and all(c > 0 for c in more['class_pairs'])
    assert got == one_share


def _small_plan(kind):
    """three pairs of about 20 letters with CIGARs -> (the plan, the dtype of its rows, its fetch in libclh)"""
    from ciri_long_amd import hip
    rng = chk.rng_for('gpu pairs plan fetch capacity')
    rs = [chk.random_seq(rng, n) for n in (20, 23, 18)]
    qs = [_copy_of(rng, r, m, rate=0.2) for r, m in zip(rs, (20, 19, 21))]
    qd, qo = hip.pack(qs); rd, ro = hip.pack(rs)
    if kind == 'ends':
        return _ctx().ends_plan(qd, qo, rd, ro, hip.score_matrix(2, 2), 3, 1), hip.ENDS_DTYPE, hip.lib().clh_ends_plan_fetch
    return _ctx().band_plan(qd, qo, rd, ro, hip.score_matrix(2, 2), 3, 1, 6), hip.BAND_DTYPE, hip.lib().clh_band_plan_fetch


@pytest.mark.parametrize('kind', ['ends', 'band'])
def test_fetch_capacity_through_the_c_abi(kind):
    from ciri_long_amd import hip
    plan, dtype, fetch = _small_plan(kind)
    try:
        plan.run()
        full_rows, full_cig = plan.fetch()
        n_ops = len(full_cig)
        assert n_ops == int(full_rows['cigar_len'].sum()) and n_ops >= 3

        def call(cap, with_buffer=True):
            rows = np.zeros(plan.n, dtype=dtype)
            cig = np.zeros(max(cap, 1), dtype=np.uint32)
            used = C.c_int64(-1)
            rc = fetch(plan._h, rows.ctypes.data, cig.ctypes.data if with_buffer else None, cap, C.byref(used))
            return rc, rows, cig, int(used.value)

        rc, rows, cig, used = call(n_ops)                        # exactly what a full fetch used
        assert rc == 0 and used == n_ops
        assert rows.tobytes() == full_rows.tobytes() and cig[:n_ops].tobytes() == full_cig.tobytes()
        rc, _, _, _ = call(n_ops - 1)
        assert rc == CLH_E_CAPACITY and hip.last_error().endswith('cigar_cap too small')
        assert hip.last_error().startswith('clh_%s_plan_fetch: ' % kind)
        rc, rows, _, used = call(0, with_buffer=False)           # no buffer: the sizes alone
        assert rc == 0 and used == n_ops
        assert rows['cigar_len'].tolist() == full_rows['cigar_len'].tolist() and rows['cigar_off'].tolist() == full_rows['cigar_off'].tolist()
    finally:
        plan.close()


def _pair_inputs():
    from ciri_long_amd import hip
    return hip.pack(['A']) + hip.pack(['A']) + (hip.score_matrix(2, 2), 3, 1)


KINDS = {       # kind -> (the smallest valid plan, whether fetch before run is refused in these words)
    'edit': (lambda ctx: ctx.edit_plan(['A'], ['C']), False),
    'edit_matrix': (lambda ctx: ctx.edit_matrix_plan([['A', 'C']]), False),
    'edit_align': (lambda ctx: ctx.edit_align_plan(['A'], ['C']), False),
    'edit_search': (lambda ctx: ctx.edit_search_plan(['A'], ['C']), False),
    'ends': (lambda ctx: ctx.ends_plan(*_pair_inputs()), True),
    'band': (lambda ctx: ctx.band_plan(*_pair_inputs(), 0), True),
}


def _flat(x):
    """a fetch result, whatever its nesting, as a list of bytes and plain values"""
    if isinstance(x, np.ndarray):
        return [x.dtype.str, x.shape, x.tobytes()]
    if isinstance(x, (list, tuple)):
        return [y for item in x for y in _flat(item)]
    return [x]


@pytest.mark.parametrize('kind', sorted(KINDS))
def test_the_run_bracket_of_every_plan_kind(kind):
    from ciri_long_amd import hip
    make, says_before_run = KINDS[kind]
    plan = make(_ctx())
    try:
        with pytest.raises(hip.ClhError, match=r'clh_%s_plan_timing: no run to time' % kind):
            plan.timing()
        if says_before_run:
            with pytest.raises(hip.ClhError, match=r'clh_%s_plan_fetch before clh_%s_plan_run' % (kind, kind)):
                plan.fetch()
        plan.run()
        assert plan.timing() > 0
        first = _flat(plan.fetch())
        plan.run()
        assert _flat(plan.fetch()) == first and plan.timing() > 0
    finally:
        plan.close()
    if kind == 'ends':
        assert first[2] == np.array([(2, 0, 0, 0, 0, 1, 0)], dtype=hip.ENDS_DTYPE).tobytes()      # 'A' on 'A': one match, 1M
