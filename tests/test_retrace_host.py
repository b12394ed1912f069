"""The recompute route of K1g on the CPU: tools/retrace_model.py (kept chunk columns, a tile with a row limit, a walk resumed chunk after
chunk) held to the definitions -- tests/ends_check.py and anchored_check.py, twopiece_check.py, spliced_check.py -- field by field and
CIGAR by CIGAR, at chunk widths of 3 and 8 columns so that every walk crosses chunk edges; and every fault the model can plant is
caught by the case set named beside it.  No GPU is touched."""
import itertools
import os
import sys

import pytest

import anchored_check as ac
import ends_check as ec
import spliced_check as sc
import twopiece_check as tc
from test_ends_host import _straddling
from test_spliced_host import _random_pairs as _spliced_pairs
from test_twopiece_host import _seeded_pairs

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
import retrace_model as mdl  # noqa: E402

GEOMS = [(3, 1), (4, 2)]                  # (cpl, lanes): chunks of 3 and of 8 columns, 1 and 2 lanes
MAT = ec.dna_matrix(2, 2)
MAT2 = ec.dna_matrix(2, 4)
ONE = [(3, 1), (2, 2), (1, 1), (2, 0)]
TWO = [(3, 2, 6, 1), (2, 2, 2, 2), (1, 1, 3, 0), (4, 2, 24, 1)]
SPL = [dict(go=3, ge=1, io=12, noncanonical=6), dict(go=3, ge=1, io=4, noncanonical=0), dict(go=2, ge=1, io=1, noncanonical=2),
       dict(go=2, ge=0, io=0, noncanonical=3, donor={'AG': 1}, acceptor={'GT': 0, 'AG': 2})]


def _want(model, q, r, costs, mode, strand=1, mat=None):
    if mat is not None:
        return sc.align(q, r, mat, costs, mode, strand)
    if model == 'one':
        return (ec if mode in ec.MODES else ac).align(q, r, MAT, costs[0], costs[1], mode)
    if model == 'two':
        return tc.align(q, r, MAT2, costs, mode)
    return sc.align(q, r, MAT, costs, mode, strand)


def _got(model, q, r, costs, mode, strand=1, geom=(3, 1), fault=None, stats=None, mat=None):
    return mdl.run(model, q, r, mat if mat is not None else (MAT2 if model == 'two' else MAT), costs, mode, strand, cpl=geom[0], lanes=geom[1], fault=fault, stats=stats)


def _seeded(model, tag, count=40):
    """encoded pairs without an empty side from the generators of the three models' own tests, and gaps astride chunk edges"""
    out = []
    if model == 'spliced':
        out = [(sc.encode(q), sc.encode(r)) for q, r in _spliced_pairs(('retrace', tag), count)]
    else:
        out = [(q, r) for q, r in _seeded_pairs(('retrace', model, tag), count, 30) if len(q) and len(r)]
    rng = ec.rng_for('retrace host', model, tag)
    for t in range(8):
        qs, rs = _straddling(rng, 8 if t & 4 else 4, 'AGT' if model == 'spliced' else 'ACGT', 'deleted' if t & 1 else 'added')
        out.append((ec.encode(qs), ec.encode(rs)))
    return out


def _exhaustive():
    words = [''.join(w) for k in range(1, 5) for w in itertools.product('AC', repeat=k)]
    return [(ec.encode(q), ec.encode(r)) for q in words for r in words]


def _costs(model):
    return ONE if model == 'one' else (TWO if model == 'two' else [sc.make_costs(**kw) for kw in SPL])


@pytest.mark.parametrize('mode', mdl.MODES)
@pytest.mark.parametrize('model', mdl.MODELS)
def test_the_model_equals_the_definition_on_seeded_pairs(model, mode):
    seen = multi = 0
    for t, (q, r) in enumerate(_seeded(model, mode)):
        costs = _costs(model)[t % 4]
        strand = 1 if t % 2 else -1
        want = ec.as_tuple(_want(model, q, r, costs, mode, strand))
        for geom in GEOMS:
            stats = {}
            got = _got(model, q, r, costs, mode, strand, geom, stats=stats)
            assert got != mdl.NO_WALK and ec.as_tuple(got) == want, (model, mode, t, geom, list(q), list(r), costs)
            # the budget is spent once: a step per CIGAR column (a spliced E or N run: per word), never more than i + j + 2 in all
            assert 0 <= stats['steps_left'] and stats['rounds'] <= stats['nchunks'] and stats['recomputed'] <= len(q) * len(r)
            seen += 1; multi += stats['rounds'] > 1
    assert seen >= 80 and multi >= 20


@pytest.mark.parametrize('model', mdl.MODELS)
def test_the_model_equals_the_definition_on_every_pair_over_ac_up_to_4_x_4(model):
    pairs = _exhaustive()
    assert len(pairs) == 900
    for k, (q, r) in enumerate(pairs):
        costs = _costs(model)[k % 4]
        for mode in mdl.MODES:
            want = ec.as_tuple(_want(model, q, r, costs, mode))
            got = _got(model, q, r, costs, mode, geom=(3, 1) if len(r) > 3 or k % 2 else (1, 2))
            assert got != mdl.NO_WALK and ec.as_tuple(got) == want, (model, mode, list(q), list(r), costs)


def _planted(pad, intron_len, lead=''):
    """two exons around an intron GT..AG behind `pad` letters -> (query, reference)"""
    e1, e2 = 'ACTCATTCAC', 'TCCATACTTA'
    return e1 + lead + e2, 'AT' * (pad // 2) + 'A' * (pad % 2) + e1 + 'GT' + 'ACT' * ((intron_len - 4) // 3) + 'C' * ((intron_len - 4) % 3) + 'AG' + e2 + 'TC'


def _fault_sets():
    rng = ec.rng_for('retrace host', 'faults')
    sets = {}
    # gaps of 5..6 letters astride the edges of chunks of 8 columns, three chunks and more: every kept slot is read
    sets['straddling'] = ('one', (3, 1), 'global', [tuple(map(ec.encode, _straddling(rng, 8, 'ACGT', 'deleted' if t & 1 else 'added'))) for t in range(12)])
    sets['straddling two'] = ('two', (3, 2, 6, 1), 'global', sets['straddling'][3])
    # spliced: an intron of 13..30 letters over chunk edges, with and without three query letters in front of it
    cases = [_planted(pad, length, lead) for pad in range(0, 9) for length in (13, 22, 30) for lead in ('', 'GGG')]
    sets['introns'] = ('spliced', sc.make_costs(go=3, ge=1, io=12, noncanonical=6), 'semiglobal', [tuple(map(sc.encode, c)) for c in cases])
    # spliced, mismatch 4 and a gap letter 1: the query's g stands against the reference's c in front of a canonical donor.  Where the N
    # run opens, T is F (the g inserted) and E ties with it, so H names E: a walk that forgets state T across the edge takes D
    # before I and returns the two ops the other way round.  Prefixes of 4..12 letters put that cell on the edges of both widths.
    # (Exons over C and T and an intron of A: no gap letter buys a match inside it.)
    e1, e2 = 'CTTCTCCTCTTC', 'TCCTTCTTCT'
    cases = [(e1[:k] + 'G' + e2, e1[:k] + 'C' + 'GT' + 'A' * 56 + 'AG' + e2 + 'TC') for k in range(4, 13)]
    sets['tie at the donor'] = ('spliced', sc.make_costs(go=1, ge=1, io=12, noncanonical=6), 'semiglobal', [tuple(map(sc.encode, c)) for c in cases], MAT2)
    return sets


FAULT_SETS = [('slot_c', 'straddling'), ('slot_c', 'straddling two'), ('slot_c', 'introns'), ('limit_short', 'straddling'), ('limit_short', 'introns'),
              ('run_dropped', 'straddling'), ('run_dropped', 'straddling two'), ('run_dropped', 'introns'), ('budget_renew', 'straddling'),
              ('budget_renew', 'introns'), ('state_t_lost', 'tie at the donor'), ('run_past_edge', 'introns'), ('chunk0_kept', 'straddling'),
              ('chunk0_kept', 'straddling two')]


@pytest.mark.parametrize('fault,name', FAULT_SETS)
def test_each_planted_fault_is_caught_by_its_case_set(fault, name):
    model, costs, mode, pairs = _fault_sets()[name][:4]
    mat = (_fault_sets()[name] + (None,))[4]
    caught = 0
    for q, r in pairs:
        want = ec.as_tuple(_want(model, q, r, costs, mode, mat=mat))
        for geom in GEOMS:
            clean, faulty = {}, {}
            good = _got(model, q, r, costs, mode, 1, geom, stats=clean, mat=mat)
            assert good != mdl.NO_WALK and ec.as_tuple(good) == want, (name, geom)
            # a budget renewed per round shows in the steps left alone: the walk of valid decisions never runs out of either
            bad = _got(model, q, r, costs, mode, 1, geom, fault=fault, stats=faulty, mat=mat)
            caught += bad == mdl.NO_WALK or ec.as_tuple(bad) != want or (faulty['steps_left'] != clean['steps_left'] and faulty['rounds'] > 1)
    assert caught > 0, (fault, name)
