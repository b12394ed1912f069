"""Reads to loci on the device (K7): a minimizer index of the resident genome, seed look-up and colinear chaining, offered beside the
external mapper -- nothing in find_bsj.py or mapper_pool.py is routed through it.  A chain names a contig, a strand and the two spans
it covers, and its first anchor in the form ``ssw_wrap.extend_anchors_genome`` takes, so that
``reads -> map_reads -> extend_anchors_genome / align_windows_spliced`` stays on the device from letters to CIGARs.

The definitions (minimizers with all ties selected, anchors, chain score, extraction) are the project's own and are not those of
minimap2: include/ciri_long_hip.h states them, tests/seed_check.py restates them in plain Python."""
from . import hip


def index(genome, k=15, w=5, max_occ=64):
    """the minimizer index of a ``hip.Genome``: every contig sketched as a sequence of its own, entries sorted by (key, position);
    a key with more than max_occ entries seeds nothing"""
    return hip.SeedIndex(genome, k=k, w=w, max_occ=max_occ)


def map_reads(index, reads, **chain_parameters):
    """reads: a list of str / int8 code arrays.  Per read the list of its chains, best first (``SeedIndex.chains`` and its parameters:
    lookback, max_gap, max_skew, min_score, min_anchors, max_chains, max_attempts), each a dict:

    contig, minus          the contig's name; True where the read maps to the minus strand
    score, anchors         the chain's score and its number of anchors
    ref_start, ref_end     the span of the contig from the first anchor's k-mer to the last one's
    query_start, query_end the span of the read AS GIVEN (on the minus strand converted back from the reverse-complemented read)
    anchor                 the chain's first anchor (lowest on the contig) as ``extend_anchors_genome`` takes it, (contig, pos,
                           query_pos): a plus-strand hit of read k-mer q on genome k-mer g is (contig, g, q); a minus-strand hit is
                           (contig, g + k, q), read position q facing the upper edge of the genome k-mer"""
    data, off = hip._packed(reads)
    chains, _ = index.chains((data, off), **chain_parameters)
    k = index.k
    out = []
    for r, mine in enumerate(chains):
        L = int(off[r + 1] - off[r])
        rows = []
        for c in mine:
            name = index.contigs[c['contig']]
            if c['minus']:
                qs, qe = L - c['y_end'], L - c['y_first']
                anchor = (name, c['x_first'] + k, L - k - c['y_first'])
            else:
                qs, qe = c['y_first'], c['y_end']
                anchor = (name, c['x_first'], c['y_first'])
            rows.append({'contig': name, 'minus': bool(c['minus']), 'score': c['score'], 'anchors': c['anchors'], 'ref_start': c['x_first'],
                         'ref_end': c['x_end'], 'query_start': qs, 'query_end': qe, 'anchor': anchor})
        out.append(rows)
    return out
