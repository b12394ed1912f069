"""The lifecycle of hip.py's handle wrappers (Plan, the edit, ends and band plans, CcsPlan, Genome) against a fake libclh that records
what is created and destroyed: close() destroys the handle once, and a wrapper whose context has closed destroys nothing (clh_destroy
has given everything back).  No GPU."""
import numpy as np
import pytest

from ciri_long_amd import hip


class FakeLib(object):
    """every clh_* call succeeds; *_create / clh_ssw_plan* return a fresh handle, *_destroy calls are recorded"""

    def __init__(self):
        self.created, self.destroyed, self._next = [], [], 0x1000

    def __getattr__(self, name):
        if not name.startswith('clh_'):
            raise AttributeError(name)
        if name == 'clh_last_error':
            return lambda: b''
        if name.endswith('_destroy'):
            return lambda h: self.destroyed.append((name, h))

        def call(*args):
            if name.endswith('_create') or name.startswith('clh_ssw_plan'):
                self._next += 16
                self.created.append((name, self._next))
                return self._next
            return 0
        return call


@pytest.fixture
def fake(monkeypatch):
    f = FakeLib()
    monkeypatch.setattr(hip, 'lib', lambda: f)
    return f


def _context():
    ctx = hip.Context.__new__(hip.Context)       # no device: the handle of a context that is open
    ctx._h, ctx.device = 0x10, 0
    return ctx


MAT = hip.score_matrix(2, 2)
PAIRS = hip.pack(['ACGT']) + hip.pack(['TACGTA'])       # queries, query_off, refs, ref_off
WRAPPERS = {
    'Plan': ('clh_plan_destroy', lambda ctx: ctx.plan([0, 4], [0, 8], MAT, 3, 1)),
    'EditPlan': ('clh_edit_plan_destroy', lambda ctx: ctx.edit_plan(['ACGT'], ['ACGA'])),
    'EditAlignPlan': ('clh_edit_align_plan_destroy', lambda ctx: ctx.edit_align_plan(['ACGT'], ['ACGA'], mode='HW', task='path')),
    'EditMatrixPlan': ('clh_edit_matrix_plan_destroy', lambda ctx: ctx.edit_matrix_plan([['ACGT', 'ACGA', 'AC']], hpc=True)),
    'EditSearchPlan': ('clh_edit_search_plan_destroy', lambda ctx: ctx.edit_search_plan(['ACG'], ['ACGTACGA'], k=1)),
    'EndsPlan': ('clh_ends_plan_destroy', lambda ctx: ctx.ends_plan(*PAIRS, MAT, 3, 1, mode='overlap')),
    'BandPlan': ('clh_band_plan_destroy', lambda ctx: ctx.band_plan(*PAIRS, MAT, 3, 1, 2, mode='semiglobal', diagonals=[1])),
    'CcsPlan': ('clh_ccs_plan_destroy', lambda ctx: ctx.ccs_plan(np.array([0, 100], dtype=np.int64))),
    'Genome': ('clh_genome_destroy', lambda ctx: hip.Genome(ctx, {'chr1': 'ACGTACGT'})),
}


@pytest.mark.parametrize('kind', sorted(WRAPPERS))
def test_close_destroys_the_handle_once(fake, kind):
    destroy, make = WRAPPERS[kind]
    w = make(_context())
    h = w._h
    assert h
    w.close()
    assert (destroy, h) in fake.destroyed
    n = len(fake.destroyed)
    w.close()
    assert len(fake.destroyed) == n
    assert w._h is None


@pytest.mark.parametrize('kind', sorted(WRAPPERS))
def test_nothing_is_destroyed_after_the_context_closed(fake, kind):
    destroy, make = WRAPPERS[kind]
    ctx = _context()
    w = make(ctx)
    h = w._h
    ctx.close()
    assert fake.destroyed == [('clh_destroy', 0x10)]
    w.close()
    del w
    assert all(hh != h for _name, hh in fake.destroyed)


def test_check_raises_in_the_message_shape_the_tests_match(fake):
    hip._check(0, 'clh_ssw_run')
    with pytest.raises(hip.ClhError, match=r'^clh_ssw_run failed \(-2\): $'):
        hip._check(-2, 'clh_ssw_run')
