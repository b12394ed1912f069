"""Edge sets for K6 (csrc/splice_scan.hip): small genomes whose candidates sit on the kernel's slice, mask, tier and launch edges.

A set is one genome of several contigs of at most 2 kb (the candidates' contigs never first, their offsets no multiple of 16), one
annotation index in the reference's layout and a list of cases.  A case is a candidate, the call it belongs to (search_extra,
shift_threshold, flags: bit 0 canonical only, bit 1 index slices; `bare`: no annotation loaded) and `expect`: what the run must meet,
in the words of oracle_lib.oracle_splice_trace.  tests/test_splice_edges_host.py proves every `expect` from the trace, holds
tools/splice_scan_model.py to the oracle on every case and shows its planted faults caught; tests/test_gpu_splice_edges.py sends the
same cases through Genome.splice_signals and compares the rows with `==`.

The background text holds no A, C, G or T (IUPAC letters, code 4 on the device, distinct as characters), so that the only donor and
acceptor dinucleotides of a contig are the ones a case plants and the flanks are equal exactly as far as a case copies them.  With
`fold` (the text as a minimap2 index holds it, for the index-slice cases) the background is N."""
import os
import random
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
import splice_scan_model as M  # noqa: E402

IUPAC = 'RYKMSWBDHV'
SETS = ('slide', 'contig_end', 'slices', 'masks', 'runs', 'pairs', 'rank', 'strands', 'params')
# the planted fault of tools/splice_scan_model.py -> the set that must catch it
FAULT_SET = {1: 'rank', 2: 'masks', 3: 'masks', 4: 'contig_end', 5: 'slide', 6: 'slices', 7: 'rank', 8: 'rank', 9: 'strands',
             10: 'slices', 11: 'slices', 12: 'slide', 13: 'strands'}
# de-novo motifs by weight on the plus strand (upstream acceptor, downstream donor) and their index
PLUS = {0: ('AG', 'GT', 0), 1: ('AG', 'GC', 1), 2: ('AG', 'AT', 4)}
# on the minus strand the reverse complements swap sides: upstream revcomp(donor), downstream revcomp(acceptor)
MINUS = {0: ('AC', 'CT', 0), 1: ('GC', 'CT', 1), 2: ('AT', 'CT', 4)}


def slide(text, S, E, cap=100):
    """align.py:477-493 on a plain string: (us_free, ds_free)"""
    ds = us = 0
    for i in range(cap):
        if E + i > len(text) or text[S:S + i] != text[E:E + i]:
            break
        ds = i
    for j in range(cap):
        if S - j < 0 or text[S - j:S] != text[E - j:E]:
            break
        us = j
    return us, ds


def junction(rng, L, S, E, up=0, down=0, us=(), ds=(), put=(), fold=False):
    """L background letters around a candidate [S, E): the `up` letters before and the `down` letters after both ends equal (as far as
    the contig reaches) and the next ones different; dinucleotides us = [(shift, 'AG')] at S + shift - 2 and ds = [(shift, 'GT')] at
    E + shift (copied to the other end where they fall into a shared flank); put = [(position, character)] last."""
    t = ['N' if fold else rng.choice(IUPAC) for _ in range(L)]
    for sh, di in us:
        t[S + sh - 2:S + sh] = di
    for k in range(1, up + 1):
        if S - k >= 0:
            t[E - k] = t[S - k]
    for k in range(down):
        if E + k < L:
            t[E + k] = t[S + k]
    for sh, di in ds:
        for k in range(2):
            p = E + sh + k
            t[p] = di[k]
            if -up <= p - E < down and p - (E - S) >= 0:
                t[p - (E - S)] = di[k]
    for a, b in ((S - up - 1, E - up - 1), (S + down, E + down)):
        if a >= 0 and b < L and t[a] == t[b]:
            t[a] = next(c for c in (('T', 'C') if fold else IUPAC) if c != t[b])
    for sh, di in us:
        assert ''.join(t[S + sh - 2:S + sh]) == di, ('upstream dinucleotide overwritten', sh, di)
    for sh, di in ds:
        assert ''.join(t[E + sh:E + sh + 2]) == di, ('downstream dinucleotide overwritten', sh, di)
    for p, c in put:
        t[p] = c
    assert len(t) == L
    return ''.join(t)


class EdgeSet(object):
    def __init__(self, name, seed):
        self.name = name
        self.rng = random.Random(seed)
        self.contigs = [('lead', ''.join(self.rng.choice(IUPAC + 'ACGTacgtN') for _ in range(37)))]
        self.at = 37
        self.index = {}
        self.cases = []

    def contig(self, text):
        assert 0 < len(text) <= 2048
        if self.at % 16 == 0:
            self.contigs.append(('pad%d' % len(self.contigs), 'K' * 5)); self.at += 5
        name = 'c%d' % len(self.contigs)
        self.contigs.append((name, text)); self.at += len(text)
        return name

    def site(self, ctg, pos, strand, kind):
        """an annotated exon `kind` ('start' / 'end') of `strand` at the 1-based position pos of ctg"""
        self.index.setdefault(ctg, {}).setdefault(pos, {}).setdefault(strand, {})[kind] = 1

    def anno(self, ctg, anchor, shift, strand='+', kind='end'):
        """the annotated site that gives `shift` at a candidate end `anchor` (align.py:507-546: starts are looked up one base further)"""
        self.site(ctg, anchor + shift + (1 if kind == 'start' else 0), strand, kind)

    def case(self, label, ctg, S, E, cb, host=0, se=10, st=3, flags=0, bare=False, **expect):
        self.cases.append({'label': '%s/%s' % (self.name, label), 'cand': (ctg, S, E, cb, host), 'se': se, 'st': st, 'flags': flags,
                           'bare': bare, 'expect': expect})
        return self.cases[-1]

    # ---- what the checkers need ----
    def text(self, ctg):
        return dict(self.contigs)[ctg]

    def offsets(self):
        out, at = {}, 0
        for name, t in self.contigs:
            out[name] = at; at += len(t)
        return out

    def contig_runs(self, ctg):
        """the annotated sites of one contig as oracle/splice_oracle.c takes them: (positions, counts[4]), 1-based"""
        return _runs({ctg: self.index.get(ctg, {})}, {ctg: 0}, {ctg: len(self.text(ctg))})

    def genome_runs(self):
        """the four genome-wide runs as K6 holds them (what hip.flatten_splice_sites must give)"""
        return _runs(self.index, self.offsets(), {n: len(t) for n, t in self.contigs})


def _runs(index, offset, length):
    runs = [set(), set(), set(), set()]
    for ctg, by_pos in index.items():
        for pos, by_strand in by_pos.items():
            if not 1 <= pos <= length[ctg]:
                continue
            for k, strand in enumerate('+-'):
                for q, kind in enumerate(('start', 'end')):
                    if kind in by_strand.get(strand, {}):
                        runs[2 * k + q].add(offset[ctg] + pos)
    runs = [sorted(r) for r in runs]
    flat = np.array([p for r in runs for p in r] or [0], dtype=np.int64)
    return flat, np.array([len(r) for r in runs], dtype=np.int64)


def split_runs(flat, cnt):
    out, at = [], 0
    for n in cnt.tolist():
        out.append(flat[at:at + n].tolist()); at += n
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# the seeded fuzz: small contigs, periodic and mixed text, sites and candidates near both ends
# ------------------------------------------------------------------------------------------------------------------------------
def fuzz_world(seed, n_contigs, per_contig, clip_bases=(0, 1, 5, 20, 21, 22), search_extra=10, fold=False):
    """-> (contigs [(name, text)], ss_index, cands [(ctg, S, E, cb, host_mask)]): contigs of 3 to 1 200 letters -- random, periodic,
    mixed case / IUPAC -- candidates with copied flanks and planted signals, annotated sites within sl + 2 of their ends, many of them
    within sl + 2 of the contig ends."""
    rng = random.Random(seed)
    contigs = [('lead', 'ACGTN' * 7 + 'AC')]
    index, cands = {}, []
    for c in range(n_contigs):
        kind = rng.random()
        L = rng.randint(3, 60) if rng.random() < 0.08 else rng.randint(60, 1200)
        if kind < 0.2:
            unit = ''.join(rng.choice('ACGT') for _ in range(rng.randint(1, 9)))
            s = list((unit * (L // len(unit) + 1))[:L])
        elif kind < 0.4:
            s = [rng.choice('ACGTacgtNnRYKM') for _ in range(L)]
        else:
            s = [rng.choice('ACGT') for _ in range(L)]
        name = 'f%d' % c
        mine = []
        for _ in range(per_contig):
            cb = rng.choice(clip_bases)
            sl = cb + search_extra
            r = rng.random()
            if L < 8 or r < 0.05:
                S = rng.randint(0, L - 1); E = rng.randint(S + 1, L)
            elif r < 0.3:
                S = rng.randint(0, min(L - 2, sl + 4)); E = rng.randint(S + 1, L)
            elif r < 0.5:
                E = L - rng.randint(0, min(L - 2, sl + 4)); S = rng.randint(0, E - 1)
            else:
                S = rng.randint(0, L - 2); E = rng.randint(S + 1, min(L, S + 400))
            if rng.random() < 0.5 and E - S > 8:
                f = rng.randint(0, min(120, E - S - 4, L - E)); b = rng.randint(0, min(120, E - S - 4 - f, S))
                s[E:E + f] = s[S:S + f]
                if b:
                    s[E - b:E] = s[S - b:S]
            if rng.random() < 0.7:
                i, j = rng.randint(-8, 8), rng.randint(-8, 8)
                us, ds = rng.choice([('AG', 'GT'), ('AC', 'CT'), ('AG', 'GC'), ('AC', 'AT'), ('AT', 'GT')])
                if S + i - 2 >= 0 and E + j + 2 <= L and S + i <= L and E + j >= 0:
                    s[S + i - 2:S + i] = us
                    s[E + j:E + j + 2] = ds
            if rng.random() < 0.45:
                for anchor in (S, E):
                    for _k in range(rng.choice([0, 1, 1, 2, 4])):
                        pos = anchor + rng.randint(-sl - 2, sl + 2)
                        if pos >= 1:
                            index.setdefault(name, {}).setdefault(pos, {}).setdefault(rng.choice('+-'), {})[rng.choice(['start', 'end'])] = 1
            mine.append((name, S, E, cb, rng.choice([0, 0, 1, 2, 3])))
        assert len(s) == L
        text = ''.join(s)
        if fold:
            text = ''.join(ch if ch in 'ACGT' else (ch.upper() if ch in 'acgt' else 'N') for ch in text)
        contigs.append((name, text))
        cands += mine
    return contigs, index, cands


# ------------------------------------------------------------------------------------------------------------------------------
# the sets
# ------------------------------------------------------------------------------------------------------------------------------
def _slide():
    s = EdgeSet('slide', 11)
    L, S, E, cb = 1400, 400, 900, 5
    for up, down in ((0, 0), (1, 0), (0, 1), (1, 1), (98, 98), (99, 99), (100, 100), (150, 150), (98, 150), (150, 98)):
        c = s.contig(junction(s.rng, L, S, E, up, down, us=[(0, 'AG')], ds=[(0, 'GT')]))
        s.case('flanks %d/%d' % (up, down), c, S, E, cb, us_free=min(up, 99), ds_free=min(down, 99), edge=0, found=1, win=(0, 0, 0, 0), sites=1)
    # the slide stopped by the contig's end, not by a difference: E = L - k, S = k, E == L, S == 0
    c = s.contig(junction(s.rng, 903, 400, 900, 0, 50))
    s.case('E = L - 3', c, 400, 900, cb, us_free=0, ds_free=3, edge=1)
    c = s.contig(junction(s.rng, 900, 3, 500, 50, 0))
    s.case('S = 3', c, 3, 500, cb, us_free=3, ds_free=0, edge=1)
    c = s.contig(junction(s.rng, 900, 400, 900, 4, 50))
    s.case('E == L', c, 400, 900, cb, us_free=4, ds_free=0, edge=1)
    c = s.contig(junction(s.rng, 900, 0, 500, 50, 4))
    s.case('S == 0', c, 0, 500, cb, us_free=0, ds_free=4, edge=1)
    # characters, not codes: a / A differ, equal IUPAC letters (N and n among them) do not
    c = s.contig(junction(s.rng, L, S, E, 6, 6, us=[(-8, 'AG')], ds=[(-8, 'GT')], put=[(S - 3, 'a'), (E - 3, 'A'), (S + 2, 'g'), (E + 2, 'G')]))
    s.case('case only', c, S, E, cb, us_free=2, ds_free=2, found=1, win=(0, -8, -8, 0))
    c = s.contig(junction(s.rng, L, S, E, 7, 7, us=[(-9, 'AG')], ds=[(-9, 'GT')], put=[(S - 4, 'N'), (E - 4, 'N'), (S + 3, 'n'), (E + 3, 'n')]))
    s.case('IUPAC', c, S, E, cb, us_free=7, ds_free=7, found=1, win=(0, -9, -9, 0))
    return s


def _contig_end():
    """sl = 15, us_free = 2, ds_free = 3; a de-novo GT-AG at (0, 0) and an annotated pair at (2, 2) that wins wherever it is consulted"""
    s = EdgeSet('contig_end', 12)
    cb, up, down = 5, 2, 3
    sl = cb + 10
    for label, S, gap, edge in (('S - sl - us_free - 2 == 0', sl + up + 2, 0, 0), ('S - sl - us_free - 2 == -1', sl + up + 1, 0, 1),
                                ('E + sl + ds_free + 2 == L', 150, 0, 0), ('E + sl + ds_free + 2 == L + 1', 150, 1, 1)):
        E = S + 200
        L = 400 if label[0] == 'S' else E + sl + down + 2 - gap
        c = s.contig(junction(s.rng, L, S, E, up, down, us=[(0, 'AG')], ds=[(0, 'GT')]))
        s.anno(c, S, 2); s.anno(c, E, 2)
        # at the contig's start the de-novo search has nothing to read (the upstream slice wraps to an empty one): its answer is none
        denovo = (0, (0, 0, 0, 0)) if label[0] == 'S' else (1, (0, 0, 0, 0))
        s.case(label, c, S, E, cb, us_free=up, ds_free=down, edge=edge, anno=1 - edge, found=denovo[0] if edge else 2, win=denovo[1] if edge else (0, 2, 2, 0))
    return s


def _slices():
    s = EdgeSet('slices', 13)
    for flags in (0, 2):
        fold = bool(flags)
        tag = ' (index)' if fold else ''
        none = (0, -1, 0, 0)
        # both slices start before the contig and end past it: wrapped and non-empty as Python slices, no sequence from an index
        t = junction(s.rng, 20, 4, 12, fold=fold, put=[(8, 'A'), (9, 'G'), (18, 'G'), (19, 'T')])
        c = s.contig(t)
        if fold:
            s.case('wrapped, non-empty' + tag, c, 4, 12, 5, flags=flags, edge=1, us=none, ds=none, short_seq=1, found=0)
        else:
            s.case('wrapped, non-empty', c, 4, 12, 5, edge=1, us=(7, 12, 1, 0), ds=(17, 3, 1, 1), short_seq=0, found=1, win=(0, -14, -14, 0))
        c = s.contig(junction(s.rng, 400, 4, 204, fold=fold, us=[(0, 'AG')], ds=[(0, 'GT')]))
        s.case('wrapped, empty' + tag, c, 4, 204, 5, flags=flags, edge=1, us=none if fold else (387, 0, 1, 0), short_seq=1, found=0)
        # a + L < 0: the start is clamped to 0
        c = s.contig(junction(s.rng, 10, 3, 7, fold=fold, put=[(1, 'A'), (2, 'G'), (3, 'G'), (4, 'T')]))
        if fold:
            s.case('start clamped' + tag, c, 3, 7, 5, flags=flags, edge=1, us=none, ds=none, short_seq=1, found=0)
        else:
            s.case('start clamped', c, 3, 7, 5, edge=1, us=(0, 10, 2, 1), ds=(2, 8, 1, 1), short_seq=0, found=1, win=(0, -14, -14, 0))
        # the end clipped, the start inside: a site at index n - 2 of the clipped slice
        c = s.contig(junction(s.rng, 400, 100, 390, fold=fold, us=[(8, 'AG')], ds=[(8, 'GT')]))
        s.case('end clipped' + tag, c, 100, 390, 5, flags=flags, edge=1, us=(83, 32, 0, 0), ds=(375, 25, 0, 1), short_seq=0, found=1, win=(0, 8, 8, 0))
        # need <= 0 (us_free >= ds_free + 2) with an empty upstream slice: not too short, nothing to find
        c = s.contig(junction(s.rng, 400, 6, 206, 4, 0, fold=fold))
        s.case('need <= 0' + tag, c, 6, 206, 0, flags=flags, edge=1, need=-2, us=none if fold else (390, 0, 1, 0), short_seq=1 if fold else 0, found=0)
        # a motif at index 0 of a slice is no site (str.find from 1), at index 1 and at index n - 2 it is one; sl = 15, both slides 0
        S, E, L = 300, 500, 800
        for label, i, j, hit in (('upstream index 0', -15, -14, 0), ('upstream index 1', -14, -14, 1), ('downstream index 0', -14, -15, 0),
                                 ('downstream index 1', -13, -14, 1), ('both at n - 2', 15, 15, 1)):
            c = s.contig(junction(s.rng, L, S, E, fold=fold, us=[(i, 'AG')], ds=[(j, 'GT')]))
            s.case(label + tag, c, S, E, 5, flags=flags, edge=0, us=(283, 32, 0, 0), ds=(485, 32, 0, 0), us_free=0, ds_free=0, found=hit,
                   win=(0, i, j, 0) if hit else (0, 0, 0, 0), sites=hit)
    # len == need and need - 1: a downstream slice wrapped to 7 letters, ds_free 5 (need 7) and 6 (need 8); cb = 0, sl = 10
    c = s.contig('RAGAGAGAKGTY')
    s.case('len == need', c, 1, 3, 0, us_free=0, ds_free=5, need=7, us=(1, 11, 1, 1), ds=(5, 7, 1, 1), short_seq=0, found=1)
    c = s.contig('RAGAGAGAGKGT')
    s.case('len == need - 1', c, 1, 3, 0, us_free=0, ds_free=6, need=8, ds=(5, 7, 1, 1), short_seq=1, found=0)
    # the same from an index: sl = 0 (cb = 0, search_extra = 0), ds_free 3 (need 5), the downstream slice [E, E + 5) ending with the
    # contig and clipped one short of it
    S, E = 300, 500
    c = s.contig(junction(s.rng, E + 5, S, E, 0, 3, us=[(2, 'AG')], ds=[(3, 'GT')], fold=True))
    s.case('len == need (index)', c, S, E, 0, se=0, flags=2, us_free=0, ds_free=3, need=5, us=(298, 5, 0, 0), ds=(500, 5, 0, 0), short_seq=0,
           found=1, win=(0, 2, 3, 0))
    c = s.contig(junction(s.rng, E + 4, S, E, 0, 3, us=[(2, 'AG')], fold=True))
    s.case('len == need - 1 (index)', c, S, E, 0, se=0, flags=2, us_free=0, ds_free=3, need=5, us=(298, 5, 0, 0), ds=(500, 4, 0, 1), short_seq=1,
           found=0)
    return s


def _masks():
    """sl = 15 (shifts -15 .. 14 are bits 0 .. 29); cb = 22: sl = 32, bit 63; cb = 23: past the masks"""
    s = EdgeSet('masks', 14)
    S, E, L = 300, 500, 800
    for strand in '+-':
        for kind in ('start', 'end'):
            for sh in (-15, 14, 15):
                c = s.contig(junction(s.rng, L, S, E))
                s.anno(c, S, sh, strand, kind); s.anno(c, E, sh, strand, kind)
                hit = sh < 15
                k = '+-'.index(strand)
                s.case('%s %s at %d' % (strand, kind, sh), c, S, E, 5, anno=1, found=2 if hit else 0, win=(k, sh, sh, 0) if hit else (0, 0, 0, 0),
                       shifts={k: ([sh], [sh]) if hit else ([], []), 1 - k: ([], [])})
    for sh in (-32, 31):
        c = s.contig(junction(s.rng, L, S, E))
        s.anno(c, S, sh, '-', 'start'); s.anno(c, E, sh, '+', 'end'); s.anno(c, S, sh, '+', 'end')
        s.case('cb 22 at %d' % sh, c, S, E, 22, anno=1, found=2, win=(0, sh, sh, 0))
    # cb = 23 (2 sl = 66): handed back where the annotation would be consulted, answered at a contig end and without annotation
    c = s.contig(junction(s.rng, L, S, E, us=[(0, 'AG')], ds=[(0, 'GT')]))
    s.anno(c, S, 1); s.anno(c, E, 1)
    s.case('cb 23', c, S, E, 23, anno=1, status=1, found=2, win=(0, 1, 1, 0))
    s.case('cb 23, no sites loaded', c, S, E, 23, bare=True, anno=0, status=0, found=1, win=(0, 0, 0, 0))
    c = s.contig(junction(s.rng, E + 20, S, E, us=[(0, 'AG')], ds=[(0, 'GT')]))
    s.anno(c, S, 1); s.anno(c, E, 1)
    s.case('cb 23 at a contig end', c, S, E, 23, edge=1, anno=0, status=0, found=1, win=(0, 0, 0, 0))
    # an end site at the last position of the previous contig is genome position ctg_off: no shift of this contig's candidates, whose
    # first window position is ctg_off + 2 at the least
    s.contig(junction(s.rng, 333, 100, 200))
    c = s.contig(junction(s.rng, L, 17, E, us=[(0, 'AG')], ds=[(0, 'GT')]))
    prev, prev_text = s.contigs[-2]
    for strand, kind in (('+', 'end'), ('+', 'start'), ('-', 'end'), ('-', 'start')):
        s.site(prev, len(prev_text), strand, kind)
    s.anno(c, E, 0)
    s.case('neighbour site at ctg_off', c, 17, E, 5, edge=0, anno=1, found=1, win=(0, 0, 0, 0), shifts={0: ([], [0]), 1: ([], [])})
    return s


def _runs_set():
    """runs of 0, 1 and 10^5 sites: every position of 51 contigs an annotated '+' exon end, one '+' start, nothing on '-'"""
    s = EdgeSet('runs', 15)
    first = None
    for k in range(51):
        c = s.contig('K' * 1000 + 'M' * 1000)
        first = first or c
        for pos in range(1, 2001):
            s.site(c, pos, '+', 'end')
    s.site(first, 301, '+', 'start')
    # every shift of both windows annotated: 2 sl entries per list (cb = 22: all 64 bits of the masks), the flanks slide 99 both ways
    for cb in (5, 22):
        sl = cb + 10
        s.case('every position, cb %d' % cb, first, 300, 700, cb, us_free=99, ds_free=99, anno=1, found=2,
               shifts={0: ([0] + list(range(-sl, sl)), list(range(-sl, sl))), 1: ([], [])})
    c = s.contig(junction(s.rng, 800, 300, 500))
    s.case('no site near', c, 300, 500, 5, anno=0, found=0)
    return s


def _pairs():
    """sl = 15, T = 8, both slides 0"""
    s = EdgeSet('pairs', 16)
    S, E, L, cb = 300, 500, 800, 5
    c = s.contig(junction(s.rng, L, S, E))
    s.anno(c, S, -4); s.anno(c, E, 4)
    s.case('|i - j| == T', c, S, E, cb, found=2, win=(0, -4, 4, 0), sites=1)
    c = s.contig(junction(s.rng, L, S, E))
    s.anno(c, S, -4); s.anno(c, E, 5)
    s.case('|i - j| == T + 1', c, S, E, cb, anno=1, found=0, sites=0, shifts={0: ([-4], [5]), 1: ([], [])})
    # annotated pairs (1, -1) and (-3, -1): the second is further from the ends (tot 4 against 2) and wins by the weight of the
    # genome's own dinucleotides, 0 / 1 / 2 for the five motifs on either strand, and loses with weight 3 for anything else
    donors, acceptors = ('GT', 'GC', 'AT', 'GT', 'AT'), ('AG', 'AG', 'AC', 'AC', 'AG')
    rc = lambda x: x[::-1].translate(str.maketrans('ACGT', 'TGCA'))      # noqa: E731
    for k, strand in enumerate('+-'):
        for m in range(5):
            us_ss, ds_ss = (acceptors[m], donors[m]) if k == 0 else (rc(donors[m]), rc(acceptors[m]))
            c = s.contig(junction(s.rng, L, S, E, us=[(-3, us_ss)], ds=[(-1, ds_ss)]))
            for sh in (1, -3):
                s.anno(c, S, sh, strand)
            s.anno(c, E, -1, strand)
            s.case('motif %d on %s' % (m, strand), c, S, E, cb, found=2, win=(k, -3, -1, 0), tier=0, key=(3, 2, (0, 1, 2, 2, 2)[m], 4), sites=2)
    for label, us_ss, ds_ss, strand in (('lower case', 'ag', 'GT', '+'), ('N', 'AG', 'NT', '+'), ('lower case on -', 'ac', 'CT', '-')):
        c = s.contig(junction(s.rng, L, S, E, us=[(-3, us_ss)], ds=[(-1, ds_ss)]))
        for sh in (1, -3):
            s.anno(c, S, sh, strand)
        s.anno(c, E, -1, strand)
        s.case(label, c, S, E, cb, found=2, win=('+-'.index(strand), 1, -1, 0), tier=0, key=(3, 2, 3, 2), sites=2)
    # no qualifying pair: the annotated shifts join the de-novo lists -- shift -sl lies below the motif range (lo = 1 - us_len)
    c = s.contig(junction(s.rng, L, S, E, ds=[(-10, 'GT')]))
    s.anno(c, S, -15)
    s.case('shift -sl joins', c, S, E, cb, us_free=0, anno=1, found=1, win=(0, -15, -10, 0), shifts={0: ([-15], []), 1: ([], [])})
    c = s.contig(junction(s.rng, L, S, E, us=[(10, 'AG')]))
    s.anno(c, E, 14, '+', 'start')
    s.case('shift sl - 1 joins', c, S, E, cb, anno=1, found=1, win=(0, 10, 14, 0), shifts={0: ([], [14]), 1: ([], [])})
    return s


def _strands():
    s = EdgeSet('strands', 18)
    S, E, L, cb = 300, 500, 800, 5
    c = s.contig(junction(s.rng, L, S, E, us=[(1, 'AC')], ds=[(-1, 'CT')]))          # GT-AG on the minus strand only
    s.case('host +, signal on -', c, S, E, cb, host=1, searched={(0, 0), (1, 1)}, found=1, win=(1, 1, -1, 0))
    s.case('host -, signal on -', c, S, E, cb, host=2, searched={(0, 1)}, found=1, win=(1, 1, -1, 0))
    s.case('host both', c, S, E, cb, host=3, searched={(0, 0), (0, 1)}, found=1, win=(1, 1, -1, 0))
    s.case('host none', c, S, E, cb, host=0, searched={(0, 0), (0, 1)}, found=1, win=(1, 1, -1, 0))
    c = s.contig(junction(s.rng, L, S, E, us=[(1, 'AG')], ds=[(-1, 'GT')]))
    s.case('host -, signal on +', c, S, E, cb, host=2, searched={(0, 1), (1, 0)}, found=1, win=(0, 1, -1, 0))
    # the minus strand reads the reverse complements with the sides swapped: GC-AG there is GC upstream, CT downstream; CT upstream and
    # GC downstream (the sides kept) is nothing
    c = s.contig(junction(s.rng, L, S, E, us=[(1, 'GC')], ds=[(-1, 'CT')]))
    s.case('GC-AG on -', c, S, E, cb, host=0, found=1, win=(1, 1, -1, 1))
    c = s.contig(junction(s.rng, L, S, E, us=[(1, 'CT')], ds=[(-1, 'GC')]))
    s.case('sides kept on -', c, S, E, cb, host=0, found=0)
    c = s.contig(junction(s.rng, L, S, E, us=[(1, 'AG')], ds=[(-1, 'GC')]))
    s.case('canonical only, GC-AG present', c, S, E, cb, flags=1, found=0, sites=0)
    s.case('all motifs, GC-AG present', c, S, E, cb, found=1, win=(0, 1, -1, 1))
    return s


def _params():
    s = EdgeSet('params', 19)
    S, E, L = 300, 500, 800
    for se, st in ((0, 0), (1, 0), (10, 7)):
        for cb in (0, 4):
            sl, T = cb + se, cb + st
            # a de-novo pair exactly T apart, another T + 1 apart; annotated shifts at -sl and sl - 1 where there are any
            c = s.contig(junction(s.rng, L, S, E, us=[(0, 'AG')], ds=[(T, 'GT')]))
            s.case('se %d st %d cb %d: T apart' % (se, st, cb), c, S, E, cb, se=se, st=st)
            c = s.contig(junction(s.rng, L, S, E, us=[(0, 'AG')], ds=[(T + 1, 'GT')]))
            s.case('se %d st %d cb %d: T + 1 apart' % (se, st, cb), c, S, E, cb, se=se, st=st, found=0)
            if sl:
                c = s.contig(junction(s.rng, L, S, E))
                s.anno(c, S, -sl); s.anno(c, E, -sl); s.anno(c, S, sl); s.anno(c, E, sl)
                s.case('se %d st %d cb %d: shift -sl' % (se, st, cb), c, S, E, cb, se=se, st=st, found=2, win=(0, -sl, -sl, 0))
    return s


def _duel(s, label, cb, A, B, winner, field, up=0, down=0):
    """Two sites on one contig and, on a contig of its own, the loser alone: the host test reads both keys from the traces and proves
    that the winner's is smaller in `field` first (0-3: the tier's key order; 'tier': by the tier) while a later field favours the
    loser ('w': one tier, the keys differ in the weight alone).  A / B = (strand, i, j, weight); winner 'A' or 'B'.  A is seen first where both are on one strand and motif."""
    S, E, L = 300, 500, 800
    rows = []
    for k, (strand, i, j, w) in enumerate((A, B)):
        u, d, m = (PLUS, MINUS)[strand][w]
        rows.append(((i, u), (j, d), (strand, i, j, m)))
    both = s.contig(junction(s.rng, L, S, E, up, down, us=[r[0] for r in rows], ds=[r[1] for r in rows]))
    lose = rows[1] if winner == 'A' else rows[0]
    alone = s.contig(junction(s.rng, L, S, E, up, down, us=[lose[0]], ds=[lose[1]]))
    win = rows[0] if winner == 'A' else rows[1]
    a = s.case(label, both, S, E, cb, found=1, win=win[2], us_free=up, ds_free=down, sites=2)
    b = s.case(label + ' (the loser alone)', alone, S, E, cb, found=1, win=lose[2], us_free=up, ds_free=down, sites=1)
    a['beats'] = (b, field)
    return a


def _rank():
    s = EdgeSet('rank', 17)
    S, E, L = 300, 500, 800
    # ---- tier 0: alt <= cb, key (clip_alt, alt, w, tot) ----
    _duel(s, 'alt == cb is tier 0', 3, (0, -2, 1, 2), (1, -1, 3, 1), 'A', 'tier')['expect'].update(tier=0, key=(0, 3, 2, 3))
    _duel(s, 'alt == cb + 1 is not', 3, (0, -3, 1, 2), (1, -1, 3, 1), 'B', 'w')['expect'].update(tier=2)
    _duel(s, 'cb == 0: i == j is tier 0', 0, (0, 2, 2, 2), (1, -1, -2, 1), 'A', 'tier')['expect'].update(tier=0, key=(0, 0, 2, 4))
    _duel(s, 'tier 0: clip_alt before alt and w', 3, (0, -3, 0, 2), (1, -1, -2, 1), 'A', 0)['expect'].update(tier=0)
    _duel(s, 'tier 0: w before tot', 3, (0, -2, -3, 0), (1, 0, 1, 1), 'A', 2)['expect'].update(tier=0)
    _duel(s, 'tier 0: tot decides last', 3, (0, -2, -3, 1), (1, 0, 1, 1), 'B', 3)['expect'].update(tier=0)
    # ---- tier 1: both shifts inside the free slide, key (alt, w, clip_alt, tot); cb = 1 ----
    _duel(s, 'tier 1: alt before w', 1, (0, 0, 2, 2), (0, 0, 4, 1), 'A', 0, 0, 8)['expect'].update(tier=1)
    _duel(s, 'tier 1: w before tot', 1, (0, 0, -4, 0), (0, 0, 4, 1), 'A', 1, 8, 6)['expect'].update(tier=1)
    _duel(s, 'tier 1: tot decides last', 1, (0, 0, -4, 1), (0, 0, 4, 1), 'B', 3, 8, 6)['expect'].update(tier=1)
    # its bounds: i, j at -us_free and ds_free are inside (tier 1 beats the lighter tier-3 site), one beyond they are not
    _duel(s, 'tier 1: i == -us_free', 1, (0, -4, 0, 2), (1, -7, -10, 1), 'A', 'tier', 4, 4)['expect'].update(tier=1)
    _duel(s, 'tier 1: i == -us_free - 1', 1, (0, -5, -1, 2), (1, -7, -10, 1), 'B', 0, 4, 4)['expect'].update(tier=3)
    _duel(s, 'tier 1: j == ds_free', 1, (0, 0, 4, 2), (1, -7, -10, 1), 'A', 'tier', 4, 4)['expect'].update(tier=1)
    _duel(s, 'tier 1: j == ds_free + 1', 1, (0, 1, 5, 2), (1, -7, -10, 1), 'B', 0, 4, 4)['expect'].update(tier=3)
    _duel(s, 'tier 1: i == ds_free', 1, (0, 4, 0, 2), (1, -7, -10, 1), 'A', 'tier', 4, 4)['expect'].update(tier=1)
    _duel(s, 'tier 1: i == ds_free + 1', 1, (0, 5, 1, 2), (1, -7, -10, 1), 'B', 0, 4, 4)['expect'].update(tier=3)
    _duel(s, 'tier 1: j == -us_free', 1, (0, 0, -4, 2), (1, -7, -10, 1), 'A', 'tier', 4, 4)['expect'].update(tier=1)
    _duel(s, 'tier 1: j == -us_free - 1', 1, (0, -1, -5, 2), (1, -7, -10, 1), 'B', 0, 4, 4)['expect'].update(tier=3)
    # ---- tier 2: -cb <= i <= 0 <= j <= cb (alt > cb), key (w, alt, clip_alt, tot) ----
    _duel(s, 'tier 2: i == -cb', 3, (0, -3, 1, 2), (1, -5, -1, 1), 'A', 'tier')['expect'].update(tier=2)
    _duel(s, 'tier 2: i == -cb - 1', 3, (0, -4, 0, 2), (1, -6, -2, 1), 'B', 0)['expect'].update(tier=3)
    _duel(s, 'tier 2: j == cb', 3, (0, -1, 3, 2), (1, -5, -1, 1), 'A', 'tier')['expect'].update(tier=2)
    _duel(s, 'tier 2: j == cb + 1', 3, (0, 0, 4, 2), (1, -5, -1, 1), 'B', 0)['expect'].update(tier=3)
    _duel(s, 'tier 2: i > 0', 3, (0, 5, 0, 2), (1, -6, -2, 1), 'B', 0)['expect'].update(tier=3)
    _duel(s, 'tier 2: j < 0', 3, (0, 0, -5, 2), (1, 5, 1, 1), 'B', 0)['expect'].update(tier=3)
    _duel(s, 'tier 2: w before alt', 3, (0, -3, 3, 1), (0, -3, 1, 2), 'A', 0)['expect'].update(tier=2)
    _duel(s, 'tier 2: alt before tot', 5, (0, -2, 5, 0), (1, -5, 3, 0), 'A', 1, 4, 0)['expect'].update(tier=2)
    _duel(s, 'tier 2: tot decides last', 3, (0, -1, 3, 1), (1, -3, 1, 1), 'B', 3, 2, 0)['expect'].update(tier=2)
    # ---- tier 3: the same key ----
    _duel(s, 'tier 3: w before alt', 3, (0, 5, 11, 1), (1, 3, 7, 2), 'A', 0)['expect'].update(tier=3)
    _duel(s, 'tier 3: alt before tot', 3, (0, 5, 9, 1), (1, -1, 4, 1), 'A', 1)['expect'].update(tier=3)
    _duel(s, 'tier 3: tot decides last', 3, (0, 5, 9, 1), (1, 1, 5, 1), 'B', 3)['expect'].update(tier=3)
    # ---- full ties: the strict comparison keeps the first seen -- strand, then motif, then i, then j ----
    c = s.contig(junction(s.rng, L, S, E, us=[(-1, 'AG'), (1, 'GC')], ds=[(1, 'GC'), (-1, 'CT')]))
    s.case('tie: + before -', c, S, E, 3, found=1, win=(0, -1, 1, 1), same_key=2, sites=2, tier=0)
    c = s.contig(junction(s.rng, L, S, E, ds=[(0, 'AT')]))
    s.anno(c, S, 0)
    s.case('tie: motif 2 before motif 4', c, S, E, 3, anno=1, found=1, win=(0, 0, 0, 2), same_key=2, sites=2, tier=0)
    c = s.contig(junction(s.rng, L, S, E, us=[(-2, 'AG'), (2, 'AG')], ds=[(0, 'GC')]))
    s.case('tie: lower i first', c, S, E, 3, found=1, win=(0, -2, 0, 1), same_key=2, sites=2, tier=0)
    c = s.contig(junction(s.rng, L, S, E, us=[(0, 'AG')], ds=[(-2, 'GC'), (2, 'GC')]))
    s.case('tie: lower j first', c, S, E, 3, found=1, win=(0, 0, -2, 1), same_key=2, sites=2, tier=0)
    for cb, sh, tier in ((3, 2, 0), (1, 3, 3)):
        c = s.contig(junction(s.rng, L, S, E))
        s.anno(c, S, sh, '+', 'start'); s.anno(c, S, -sh, '+', 'end'); s.anno(c, E, 0)
        s.case('tie: annotated starts before ends, tier %d' % tier, c, S, E, cb, found=2, win=(0, sh, 0, 0), same_key=2, sites=2, tier=tier,
               shifts={0: ([sh, -sh], [0]), 1: ([], [])})
    return s


BUILDERS = {'slide': _slide, 'contig_end': _contig_end, 'slices': _slices, 'masks': _masks, 'runs': _runs_set, 'pairs': _pairs, 'rank': _rank,
            'strands': _strands, 'params': _params}
_built = {}


def build(name):
    """the set `name` (built once: the tests share it and leave it unchanged)"""
    if name not in _built:
        _built[name] = BUILDERS[name]()
    return _built[name]


# ------------------------------------------------------------------------------------------------------------------------------
# the answers the GPU rows are compared with
# ------------------------------------------------------------------------------------------------------------------------------
def oracle_row(s, case, trace=False):
    """oracle/splice_oracle.c on one case of the set s: the row of eight (and the trace)"""
    import oracle_lib
    ctg, S, E, cb, host = case['cand']
    f = oracle_lib.oracle_splice_trace if trace else oracle_lib.oracle_splice_row
    return f(s.text(ctg), S, E, cb, host, case['flags'] & 1, None if case['bare'] else s.contig_runs(ctg), bool(case['flags'] & 2), case['se'],
             case['st'])


def kernel_row(case, row):
    """what K6 must write where the oracle's row is `row`: the same, but for the candidates it hands back (expect status 1), which
    keep only the slides"""
    return [1, row[1], row[2], 0, 0, 0, 0, 0] if case['expect'].get('status') == 1 else row


class TextGenome(object):
    """the genome as the reference's Fasta serves it: Python slices of the contig's text"""

    def __init__(self, contigs):
        self.genome = dict(contigs)
        self.contig_len = {k: len(v) for k, v in self.genome.items()}

    def seq(self, ctg, start, end):
        g = self.genome.get(ctg)
        return None if g is None else g[start:end]


def mirror_row(s, case):
    """the Python statement of the step (ciri_long_amd/align.py: find_annotated_signal, then find_denovo_signal) as a row of eight"""
    import oracle_lib
    from ciri_long_amd import align, env
    ctg, S, E, cb, host = case['cand']
    env.initializer(None, {n: len(t) for n, t in s.contigs}, TextGenome(s.contigs), None, None, None if case['bare'] else (s.index or None))
    sl = cb + case['se']
    site, us_free, ds_free, sig = align.find_annotated_signal(ctg, S, E, cb, sl, case['st'])
    found = 2 if site is not None else 0
    if site is None:
        hosts = {st: 1 for k, st in enumerate('+-') if (host >> k) & 1} or None
        site = align.find_denovo_signal(ctg, S, E, hosts, sig, us_free, ds_free, cb, sl, case['st'], bool(case['flags'] & 1))
        found = 1 if site is not None else 0
    row = [0, us_free, ds_free, found, 0, 0, 0, 0]
    if site is not None:
        ident, strand, i, j = site
        motif = 0
        if found == 1:
            acceptor, donor = ident.split('*')[0].split('-')
            motif = oracle_lib._SPLICE_MOTIFS.index((donor, acceptor))
        row[4:8] = ['+-'.index(strand), i, j, motif]
    return row
