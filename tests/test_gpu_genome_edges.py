"""K5 (genome.hip) at its block, tail and byte-value edges.  The comparison is a plain table (A/a 0, C/c 1, G/g 2, T/t 3, anything
else N; lower case only for acgt; N only for 'N') and str.count('N').

What is resident is seen through the entry points that read it: the codes through `global` pair plans on windows (the gather), the N
flag through count_n, the lower-case flag through a minus-strand ssw_windows row and through K6's flank comparison.

Seeing the codes: a window of the genome is aligned end to end with the string the table gives for it, every N of that string
replaced by one letter, once per letter.  All four scores equal twice the number of table bases exactly when the window holds the
table's codes: a wrong base loses a match in every pass, a base where the table says N wins one in the pass of its letter, an N where
the table says a base loses one."""
import numpy as np
import pytest

gpu = pytest.mark.gpu

BLOCK = 256                  # bases per entry of the N prefix table (clh_device.h: kGenomeBlock)
ENCODE_GROUP = 4096          # bases per workgroup of the encode kernel, 16 per thread
LENGTHS = [1, 15, 16, 17, 255, 256, 257, 4095, 4096, 4097, 8192 + 3]
CODE = {c: k for k, c in enumerate('ACGT')}


def table(text):
    """the string the byte table gives: upper-case base or N"""
    return ''.join(c.upper() if c in 'ACGTacgt' else 'N' for c in text)


def test_constants_are_the_sources():
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'ciri_long_amd', 'csrc')
    assert int(re.search(r'static constexpr int kGenomeBlock = (\d+);', open(os.path.join(csrc, 'clh_device.h')).read()).group(1)) == BLOCK
    assert 'const long long per = 256ll * 16;' in open(os.path.join(csrc, 'genome.hip')).read() and ENCODE_GROUP == 256 * 16


def codes_equal_table(ctx, g, text, chunk=509):
    """every byte of the resident genome against table(text), in windows of `chunk` bases (no multiple of 16), four passes in one plan"""
    from ciri_long_amd import hip
    want = table(text)
    spans = [(a, min(len(text), a + chunk)) for a in range(0, len(text), chunk)]
    queries, off, ln, expect = [], [], [], []
    for a, b in spans:
        for letter in 'ACGT':
            queries.append(want[a:b].replace('N', letter))
            off.append(a); ln.append(b - a)
            expect.append(2 * (b - a - want[a:b].count('N')))
    qd, qo = hip.pack(queries)
    rows, _cig = ctx.ends_batch(qd, qo, None, None, hip.score_matrix(2, 2), 3, 1, mode='global', want_cigar=False,
                                windows=(g, np.array(off, dtype=np.int64), np.array(ln, dtype=np.int64), np.zeros(len(off), dtype=np.uint8)))
    got = [int(r['score']) for r in rows]
    assert got == expect, [(k // 4, 'ACGT'[k % 4], g_, e) for k, (g_, e) in enumerate(zip(got, expect)) if g_ != e][:5]


def edge_points(n):
    """0, the length and the three positions around every block edge inside"""
    pts = {0, n}
    for k in range(1, n // BLOCK + 2):
        pts |= {p for p in (BLOCK * k - 1, BLOCK * k, BLOCK * k + 1) if 0 <= p <= n}
    return sorted(pts)


def count_n_equals_str_count(g, text):
    """every window (s, e) between edge points: the empty ones, the ones inside one block, sb == eb, whole blocks between, the whole genome"""
    pts = edge_points(len(text))
    wins = [(s, e) for s in pts for e in pts if s <= e]
    got = g.count_n_spans(np.array([s for s, _ in wins], dtype=np.int64), np.array([e - s for s, e in wins], dtype=np.int64)).tolist()
    assert got == [text[s:e].count('N') for s, e in wins]
    return wins


def split(text):
    """contigs whose boundaries are no block edge and no multiple of 16"""
    cuts = [c for c in (7, 100, 1001, 4099, 6007) if c < len(text)]
    edges = [0] + cuts + [len(text)]
    return [('k%d' % i, text[a:b]) for i, (a, b) in enumerate(zip(edges, edges[1:])) if b > a]


@gpu
@pytest.mark.parametrize('n', LENGTHS)
def test_genome_lengths_around_the_tail_the_block_and_the_workgroup(n):
    from ciri_long_amd import hip
    rng = np.random.default_rng(1000 + n)
    alphabet = 'ACGTacgtNnRYKM-*'
    t = [alphabet[i] for i in rng.integers(0, len(alphabet), n)]
    for p in edge_points(n):                           # N at the first and last byte of every block and on both sides of every edge
        if 0 < p < n and p % BLOCK != 1:
            t[p] = 'N'
    t[0] = 'N'; t[n - 1] = 'N' if n > 1 else t[0]
    text = ''.join(t)
    contigs = split(text)
    assert ''.join(s for _, s in contigs) == text and all((sum(len(s) for _, s in contigs[:k]) % 16) for k in range(1, len(contigs)))
    ctx = hip.default_context()
    g = hip.Genome(ctx, contigs)
    codes_equal_table(ctx, g, text)
    wins = count_n_equals_str_count(g, text)
    assert (0, 0) in wins and (0, n) in wins and (n, n) in wins
    # the same through contig coordinates
    cw = [(name, 0, len(s)) for name, s in contigs] + [(name, len(s) // 2, len(s)) for name, s in contigs]
    assert g.count_n(cw).tolist() == [dict(contigs)[c][a:b].count('N') for c, a, b in cw]
    g.close()


def test_count_n_takes_each_of_its_three_branches():
    """host arithmetic of genome_count_n_kernel on the windows above: inside one block (no whole block, sb > eb), sb == eb (two edge
    loops, no table difference), sb < eb (table difference), and the empty window"""
    n = LENGTHS[-1]
    pts = edge_points(n)
    seen = set()
    for s in pts:
        for e in pts:
            if s > e:
                continue
            sb, eb = (s + BLOCK - 1) // BLOCK, e // BLOCK
            seen.add('empty' if e == s else 'inside' if sb > eb else 'touching' if sb == eb else 'blocks')
            if s < e and sb <= eb:
                seen.add(('head', sb * BLOCK - s)); seen.add(('tail', e - eb * BLOCK))
    assert {'empty', 'inside', 'touching', 'blocks', ('head', 0), ('head', 1), ('head', BLOCK - 1), ('tail', 0), ('tail', 1), ('tail', BLOCK - 1)} <= seen
    assert n % 16 == 3 and n > 2 * ENCODE_GROUP and {ENCODE_GROUP - 1, ENCODE_GROUP, ENCODE_GROUP + 1} <= set(LENGTHS)


@gpu
def test_all_256_byte_values():
    from ciri_long_amd import hip
    every = ''.join(chr(b) for b in range(256))
    contigs = [('lead', 'acgtN' * 5 + 'ag'), ('bytes', every), ('again', every[::-1] + 'ACG')]
    text = ''.join(s for _, s in contigs)
    ctx = hip.default_context()
    g = hip.Genome(ctx, contigs)
    # the code of every byte: a one-base window against each of the four bases
    off = np.repeat(np.arange(len(text), dtype=np.int64), 4)
    qd = np.tile(np.arange(4, dtype=np.int8), len(text))
    qo = np.arange(4 * len(text) + 1, dtype=np.int64)
    rows, _cig = ctx.ends_batch(qd, qo, None, None, hip.score_matrix(2, 2), 3, 1, mode='global', want_cigar=False,
                                windows=(g, off, np.ones(len(off), dtype=np.int64), np.zeros(len(off), dtype=np.uint8)))
    score = np.array([int(r['score']) for r in rows]).reshape(len(text), 4)
    for p, ch in enumerate(text):
        want = [0, 0, 0, 0]
        if ch in 'ACGTacgt':
            want = [2 if k == CODE[ch.upper()] else -2 for k in range(4)]
        assert score[p].tolist() == want, (p, ord(ch), score[p].tolist())
    assert sorted(ord(c) for c in set(every) if table(c) != 'N') == sorted(ord(c) for c in 'ACGTacgt')
    # the N flag: 'N' alone, byte by byte and over the whole
    ones = g.count_n_spans(np.arange(len(text), dtype=np.int64), np.ones(len(text), dtype=np.int64)).tolist()
    assert ones == [1 if c == 'N' else 0 for c in text] and sum(ones) == 7
    count_n_equals_str_count(g, text)
    codes_equal_table(ctx, g, text, chunk=61)
    g.close()


@gpu
def test_lower_case_flag_through_a_minus_strand_window_and_through_flanks():
    """revcomp() complements upper case only: a lower-case base of a minus-strand window is reversed, not complemented.  And K6 compares
    flanks as characters: a / A end the slide."""
    import oracle_lib
    import splice_edges as E
    from ciri_long_amd import hip
    from ciri_long_amd.utils import revcomp
    rng = np.random.default_rng(5)
    body = ''.join('ACGTacgt'[i] for i in rng.integers(0, 8, 333))
    contigs = [('pad', 'NNNNNNN'), ('mixed', body)]
    ctx = hip.default_context()
    g = hip.Genome(ctx, contigs)
    wins = [('mixed', 0, 333), ('mixed', 9, 265), ('mixed', 250, 333)]
    strings = [revcomp(body[a:b]) for _c, a, b in wins]
    assert all(any(c.islower() for c in s) for s in strings)
    full = [body[a:b].upper()[::-1].translate(str.maketrans('ACGT', 'TGCA')) for _c, a, b in wins]      # were every base complemented
    reads = [s.upper() for s in strings]
    data, off = hip.pack(reads)
    rows, _c = g.ssw_windows(data, off, wins, np.ones(len(wins), dtype=np.uint8), hip.score_matrix(1, 1), 1, 1)
    for s, q, f, r in zip(strings, reads, full, rows):
        want = oracle_lib.oracle_align(s, q, 1, 1, 1, 1)
        assert (int(r['score1']), int(r['ref_begin1']), int(r['ref_end1'])) == (want['score'], want['ref_begin'], want['ref_end'])
        assert int(r['score1']) == len(q) > oracle_lib.oracle_align(f, q, 1, 1, 1, 1)['score']
    g.close()
    s = E.build('slide')
    case = [c for c in s.cases if c['label'] == 'slide/case only'][0]
    dev = hip.Genome(ctx, s.contigs)
    row = dev.splice_signals([case['cand']], 10, 3, False).tolist()[0]
    dev.close()
    assert row == E.oracle_row(s, case) and (row[1], row[2]) == (2, 2)
