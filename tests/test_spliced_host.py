"""Spliced pair alignment on the CPU: the definition (tests/spliced_check.py) against the enumeration of every global alignment with
each maximal run of skipped reference letters costed by the one rule, against itself (cell by cell and row by row), and the scheme of
the kernel (tools/spliced_model.py, run with few lanes and small chunks) against the definition, with planted faults that named case
sets catch; a literal three-exon case; and the wrapper's argument errors, which are raised before any device is touched."""
import itertools
import os
import sys

import pytest

import spliced_check as chk

TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools')
sys.path.insert(0, TOOLS)
import spliced_model as mdl  # noqa: E402

MAT = chk.dna_matrix(2, 2)
# (go, ge, io, noncanonical): the second makes a deletion of two letters and an intron tie (3 + 1 == 4 + 0 + 0); the third makes
# introns cheap enough to compete with single mismatches, the fourth has sites that matter and a free extension
SMALL = [dict(go=3, ge=1, io=12, noncanonical=6), dict(go=3, ge=1, io=4, noncanonical=0), dict(go=2, ge=1, io=1, noncanonical=2),
         dict(go=2, ge=0, io=0, noncanonical=3, donor={'AG': 1}, acceptor={'GT': 0, 'AG': 2})]
GEOMS = [(2, 4), (1, 3), (4, 2)]       # (cpl, lanes): chunks of 8, 3 and 8 columns


def _words(alphabet, max_len, min_len=0):
    return [''.join(w) for n in range(min_len, max_len + 1) for w in itertools.product(alphabet, repeat=n)]


# ---- the enumeration ---------------------------------------------------------------------------------------------------------
def _global_paths(m, n):
    """every global alignment of an m x n pair -> [(M cells, D runs as (a, b) 0-based inclusive, I run lengths)]; ops in every order,
    a maximal run of one op is one run"""
    out = []

    def go(i, j, cells, druns, iruns, last):
        if (i, j) == (m, n):
            out.append((tuple(cells), tuple(druns), tuple(iruns)))
            return
        if i < m and j < n:
            go(i + 1, j + 1, cells + [(i, j)], druns, iruns, 'M')
        if j < n:
            go(i, j + 1, cells, druns[:-1] + [(druns[-1][0], j)] if last == 'D' else druns + [(j, j)], iruns, 'D')
        if i < m:
            go(i + 1, j, cells, druns, iruns[:-1] + [iruns[-1] + 1] if last == 'I' else iruns + [1], 'I')
    go(0, 0, [], [], [], None)
    return out


_PATHS = {}


def _best_global(q, r, costs, strand):
    m, n = len(q), len(r)
    if (m, n) not in _PATHS:
        _PATHS[(m, n)] = _global_paths(m, n)
    go, ge = costs[:2]
    don, acc = chk.site_costs(r, costs, strand)
    best = None
    for cells, druns, iruns in _PATHS[(m, n)]:
        v = sum(int(MAT[r[j]][q[i]]) for i, j in cells) - sum(go + (k - 1) * ge for k in iruns)
        v -= sum(min(chk.run_costs(a, b, costs, don, acc)) for a, b in druns)
        best = v if best is None or v > best else best
    return best


@pytest.mark.parametrize('strand', [1, -1])
@pytest.mark.parametrize('kw', SMALL)
def test_plain_is_the_best_over_every_global_alignment_with_each_run_costed_by_the_rule(kw, strand):
    """every query over AG up to 3 letters x every reference over AGT up to 5 letters; the score is the enumeration's, the CIGAR
    rescores to it, and a run is N only where the intron is strictly cheaper: a tie is D"""
    costs = chk.make_costs(**kw)
    count = 0
    for qs in _words('AG', 3):
        q = chk.encode(qs)
        for rs in _words('AGT', 5):
            r = chk.encode(rs)
            res = chk.plain(q, r, MAT, costs, 'global', strand)
            assert res['score'] == _best_global(q, r, costs, strand), (qs, rs, kw, strand)
            chk.check_cigar(res, q, r, MAT, costs, 'global', strand)
            don, acc = chk.site_costs(r, costs, strand)
            j = 0
            for op, k in res['cigar']:
                if op in 'DN':
                    d, x = chk.run_costs(j, j + k - 1, costs, don, acc)
                    assert (op == 'D' and d <= x) or (op == 'N' and x < d), (qs, rs, res['cigar'])
                j += k if op != 'I' else 0
            count += 1
    assert count == 15 * 364


def test_a_tie_between_a_deletion_and_an_intron_is_a_deletion():
    costs = chk.make_costs(**SMALL[1])
    q, r = chk.encode('AGGA'), chk.encode('AGTTGA')
    for strand in (1, -1):
        assert chk.as_tuple(chk.plain(q, r, MAT, costs, 'global', strand)) == (4, 0, 5, 0, 3, '2M2D2M')
        assert chk.as_tuple(chk.align(q, r, MAT, costs, 'global', strand)) == (4, 0, 5, 0, 3, '2M2D2M')
    # row 0: two leading letters, a tie again
    assert chk.as_tuple(chk.plain(chk.encode('GA'), chk.encode('TTGA'), MAT, costs, 'global'))[5] == '2D2M'
    # one letter dearer as a deletion: the intron
    assert chk.as_tuple(chk.plain(q, chk.encode('AGTTTGA'), MAT, costs, 'global'))[5] == '2M3N2M'


# ---- align == plain == the model -----------------------------------------------------------------------------------------------
def _random_pairs(key, count, max_m=9, max_n=26):
    rng = chk.rng_for('spliced host', key)
    out = []
    for _ in range(count):
        n = rng.randint(1, max_n)
        rs = chk.random_seq(rng, n, 'AGTAGTN' if rng.random() < 0.3 else 'AGT')
        if rng.random() < 0.6 and n >= 4:      # a spliced copy: two or three stretches of the reference, mutated
            cuts = sorted(rng.sample(range(n + 1), min(n + 1, rng.choice((4, 6)))))
            qs = ''.join(rs[a:b] for a, b in zip(cuts[::2], cuts[1::2])).replace('N', 'A')
            qs = chk.mutate(rng, qs, 0.1, 'AGT')[:max_m]
        else:
            qs = chk.random_seq(rng, rng.randint(1, max_m), 'AGT')
        out.append((qs or 'A', rs))
    return out


@pytest.mark.parametrize('mode', chk.MODES)
def test_align_plain_and_the_model_agree_on_random_pairs(mode):
    n_pairs = 0
    for c, kw in enumerate(SMALL):
        costs = chk.make_costs(**kw)
        for k, (qs, rs) in enumerate(_random_pairs((mode, c), 90)):
            q, r = chk.encode(qs), chk.encode(rs)
            strand = 1 if k % 2 else -1
            want = chk.as_tuple(chk.plain(q, r, MAT, costs, mode, strand))
            res = chk.align(q, r, MAT, costs, mode, strand)
            assert chk.as_tuple(res) == want, (qs, rs, kw, strand)
            chk.check_cigar(res, q, r, MAT, costs, mode, strand)
            cpl, lanes = GEOMS[k % len(GEOMS)]
            assert chk.as_tuple(mdl.run(q, r, MAT, costs, mode, strand, cpl=cpl, lanes=lanes)) == want, (qs, rs, kw, strand, cpl, lanes)
            only = chk.align(q, r, MAT, costs, mode, strand, path=False)
            got = mdl.run(q, r, MAT, costs, mode, strand, cpl=cpl, lanes=lanes, store=False)
            assert (only['score'], only['ref_end'], only['query_end']) == (got['score'], got['ref_end'], got['query_end']) == (want[0], want[2], want[4])
            n_pairs += 1
    assert n_pairs == 360


def test_the_model_at_the_kernel_s_geometry():
    rng = chk.rng_for('spliced host', 'full geometry')
    costs = chk.make_costs()
    e1, e2 = chk.random_seq(rng, 12), chk.random_seq(rng, 12)
    rs = chk.random_seq(rng, 5) + e1 + 'GT' + chk.random_seq(rng, 520, 'ACT') + 'AG' + e2 + chk.random_seq(rng, 3)
    q, r = chk.encode(e1 + e2), chk.encode(rs)
    for mode in ('semiglobal', 'global'):
        want = chk.align(q, r, MAT, costs, mode)
        assert ('524N' in chk.cigar_text(want['cigar']))
        assert chk.as_tuple(mdl.run(q, r, MAT, costs, mode)) == chk.as_tuple(want)


# ---- planted faults ------------------------------------------------------------------------------------------------------------
def _planted(pad, intron_len, strand=1, lead='', tail='TCA'):
    """exon + intron + exon on the given strand, `pad` letters in front -> (query, reference): the intron is canonical"""
    e1, e2 = 'ACGTTACGTC', 'TCCATGCAAT'      # the exon does not end in A: the intron's first letter G closes no AG
    intron = 'GT' + ('ACT' * intron_len)[:intron_len - 4] + 'AG'
    rs = 'CCTAATCG'[:pad] + lead + e1 + intron + e2 + tail
    qs = e1 + e2
    if strand < 0:
        comp = {'A': 'T', 'C': 'G', 'G': 'C', 'T': 'A'}
        rs = ''.join(comp[c] for c in reversed(rs)); qs = ''.join(comp[c] for c in reversed(qs))
    return qs, rs


CASES = {
    # a canonical intron at every offset against the lanes: its sites decide the score
    'sites': [(m, s) + _planted(p, 14, s) for p in range(8) for m in ('semiglobal', 'global') for s in (1, -1)],
    # an intron longer than a chunk of 8 columns: N crosses hand-overs
    'long': [('semiglobal', 1) + _planted(p, 30) for p in range(8)],
    # one more letter in front of the donor: only a deletion next to the intron would spare the noncanonical donor
    'adjacent': [('semiglobal', 1, 'ACGTTACGGA' + 'TCCATGCAAT', 'CCTAATCG'[:p] + 'ACGTTACGGA' + 'C' + 'GT' + 'ACTACTACTA' + 'AG' + 'TCCATGCAAT' + 'TCA') for p in range(8)],
    # a leading intron in an anchored mode: row 0
    'row0': [(m, 1, 'TCCATGCAAT', 'GT' + 'ACT' * 8 + 'AG' + 'TCCATGCAAT' + t) for m, t in (('global', ''), ('prefix', 'CA'), ('extend', 'CA'))],
}


def _mismatches(cases, costs, fault, geoms=GEOMS):
    bad = 0
    for mode, strand, qs, rs in cases:
        q, r = chk.encode(qs), chk.encode(rs)
        want = chk.as_tuple(chk.align(q, r, MAT, costs, mode, strand))
        for cpl, lanes in geoms:
            bad += chk.as_tuple(mdl.run(q, r, MAT, costs, mode, strand, cpl=cpl, lanes=lanes, fault=fault)) != want
    return bad


def _tie_cases():
    return [('global', s, qs, rs) for s in (1, -1) for qs in _words('AG', 2, 1) for rs in _words('AGT', 4, 1)]


@pytest.mark.parametrize('fault, name, kw', [
    ('donor_off', 'sites', SMALL[0]), ('acc_at_open', 'sites', SMALL[0]), ('handover_n', 'long', SMALL[0]), ('open_from_h', 'adjacent', SMALL[0]),
    ('tie_flip', 'tie', SMALL[1]), ('minus_plain', 'sites', SMALL[0]), ('row0_plain', 'row0', SMALL[0])])
def test_each_planted_fault_is_caught_by_its_case_set(fault, name, kw):
    costs = chk.make_costs(**kw)
    cases = _tie_cases() if name == 'tie' else CASES[name]
    assert _mismatches(cases, costs, None) == 0
    assert _mismatches(cases, costs, fault) > 0, fault
    assert set(mdl.FAULTS) == {'donor_off', 'acc_at_open', 'handover_n', 'open_from_h', 'tie_flip', 'minus_plain', 'row0_plain'}


# ---- a literal case ------------------------------------------------------------------------------------------------------------
EXONS = ('ACGTTACGGATCCATGCAAT', 'TTCGAGGCTAACCGTATGCA', 'GGATTCACCGTAGCTAGCAT')


def literal_case():
    rng = chk.rng_for('spliced literal')
    i1 = 'GT' + chk.random_seq(rng, 493, 'ACT') + 'AG'
    i2 = 'GT' + chk.random_seq(rng, 696, 'ACT') + 'AG'
    return ''.join(EXONS), 'CCTA' + EXONS[0] + i1 + EXONS[1] + i2 + EXONS[2] + 'TTAC'


def revcomp(s):
    return ''.join({'A': 'T', 'C': 'G', 'G': 'C', 'T': 'A', 'N': 'N'}[c] for c in reversed(s))


def test_three_exons_against_a_window_with_two_introns():
    qs, rs = literal_case()
    assert len(rs) == 4 + 60 + 497 + 700 + 4
    costs = chk.make_costs(go=3, ge=1, io=12, noncanonical=6)
    res = chk.align(chk.encode(qs), chk.encode(rs), MAT, costs, 'semiglobal')
    assert (res['score'], res['ref_begin'], chk.cigar_text(res['cigar'])) == (96, 4, '20M497N20M700N20M')
    q2, r2 = chk.encode(revcomp(qs)), chk.encode(revcomp(rs))
    minus = chk.align(q2, r2, MAT, costs, 'semiglobal', -1)
    assert (minus['score'], minus['ref_begin'], chk.cigar_text(minus['cigar'])) == (96, 4, '20M700N20M497N20M')
    assert chk.align(q2, r2, MAT, costs, 'semiglobal', 1, path=False)['score'] < 96
    assert chk.as_tuple(mdl.run(q2, r2, MAT, costs, 'semiglobal', -1)) == chk.as_tuple(minus)


# ---- the wrapper's argument errors -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kw, text', [
    (dict(matrix=[[1]], alphabet='A'), 'CLH_E_UNSUPPORTED'), (dict(gap_open2=24, gap_extend2=1), 'CLH_E_UNSUPPORTED'),
    (dict(strand='x'), 'strand must be'), (dict(strand=['+']), 'strand must be'), (dict(intron_open=-1), 'must not be negative'),
    (dict(noncanonical=-2), 'must not be negative'), (dict(gap_open=-3), 'must not be negative'), (dict(donor_costs={'GC': -1}), 'must not be negative'),
    (dict(donor_costs={'GN': 2}), 'dinucleotides over ACGT'), (dict(acceptor_costs={'AGG': 2}), 'dinucleotides over ACGT'), (dict(mode='local'), 'mode must be')])
def test_the_wrapper_refuses_before_it_touches_a_device(kw, text):
    from ciri_long_amd import ssw_wrap
    with pytest.raises(ValueError, match=text):
        ssw_wrap.align_pairs_spliced(['ACGT', 'ACGT'], ['AC', 'GT'], **kw)


def test_the_default_tables_and_the_overrides():
    from ciri_long_amd import hip
    sp = hip.splice_of('t', 12, 6, {'GC': 2}, {'ag': 1})
    want = chk.make_costs(3, 1, 12, 6, {'GC': 2}, {'AG': 1})
    assert (sp.intron_open, tuple(sp.donor), tuple(sp.acceptor), sp.other) == want[2:]
    assert sp.donor[4 * 2 + 3] == 0 and sp.donor[4 * 2 + 1] == 2 and sp.acceptor[2] == 1
