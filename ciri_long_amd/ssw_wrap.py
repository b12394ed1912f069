"""Drop-in counterpart of the reference's ``libs/striped_smith_waterman/ssw_wrap.py`` on top of libclh.so.

Same public surface (class and attribute names, defaults, ``None`` conventions) so that CIRI-long's call sites run
unchanged:

    Aligner(ref_seq="", match=2, mismatch=2, gap_open=3, gap_extend=1, report_secondary=False, report_cigar=False)
        .align(query_seq, min_score=0, min_len=0) -> PyAlignRes | None          (ssw_wrap.py:174-230)
    PyAlignRes: score, ref_begin, ref_end, query_begin, query_end, score2, ref_end2, cigar_string   (ssw_wrap.py:315-345)

Differences, all additive:
  * the arithmetic runs on the GPU (HIP kernels behind the batched C ABI); nothing is computed on the CPU;
  * ``Aligner.align_batch(queries)`` and the module-level ``align_pairs(refs, queries, ...)`` issue ONE call for many
    alignments -- what a GPU needs, and what ``find_bsj.align_clip_segments`` / ``collapse`` are restructured around;
  * sequences are encoded with a 256-entry table instead of the reference's per-base Python loop (ssw_wrap.py:234-252);
    the resulting codes are identical (A/a 0, C/c 1, G/g 2, T/t 3, everything else 4);
  * ``align_pairs_ends`` aligns pairs end to end instead of locally -- ``mode`` 'global', 'semiglobal' (the whole query in any stretch
    of the reference) or 'overlap' (end gaps free on both sequences), and start-anchored 'prefix' or 'extend' (pinned at the
    first letters, free at the far end) -- under the same affine scores, DNA or matrix (K1g); ``extend_anchors`` extends both
    ways from an anchor between letters;
  * ``align_windows_ends``, ``align_windows_band``, ``align_windows_spliced`` and ``extend_anchors_genome`` are the pair calls with
    references given as windows (contig, start, end) of a genome resident on the GPU, gathered on the device;
  * ``align_pairs_matrix`` aligns over any alphabet of up to 32 letters with its own substitution matrix (``BLOSUM62`` for
    proteins), what the reference's ssw_init / ssw_align take and its Python wrapper does not expose.
"""
import numpy as np

from . import hip

_OPS = 'MIDNSHP=X'


class CAlignRes(object):
    """Field-for-field view of one result row (the reference's ctypes mirror of s_align, ssw_wrap.py:20-37)."""
    __slots__ = ('score', 'score2', 'ref_begin', 'ref_end', 'query_begin', 'query_end', 'ref_end2', 'cigar', 'cigarLen')

    def __init__(self, row, cigar):
        self.score = int(row['score1'])
        self.score2 = int(row['score2'])
        self.ref_begin = int(row['ref_begin1'])
        self.ref_end = int(row['ref_end1'])
        self.query_begin = int(row['read_begin1'])
        self.query_end = int(row['read_end1'])
        self.ref_end2 = int(row['ref_end2'])
        self.cigar = cigar
        self.cigarLen = len(cigar)


class PyAlignRes(object):
    """Result object with the attributes CIRI-long reads (find_bsj.py:206-224, collapse.py:157,214,256,264,382,774,
    align.py:804-806)."""

    def __init__(self, res, query_len, report_secondary=False, report_cigar=False):
        self.score = res.score
        self.ref_begin = res.ref_begin
        self.ref_end = res.ref_end
        self.query_begin = res.query_begin
        self.query_end = res.query_end
        if report_secondary and res.score2 != 0:      # ssw_wrap.py:332-338
            self.score2 = res.score2
            self.ref_end2 = res.ref_end2
        else:
            self.score2 = None
            self.ref_end2 = None
        if report_cigar and res.cigarLen > 0:          # ssw_wrap.py:341-345
            self.cigar_string = self._cigar_string(res.cigar, query_len)
        else:
            self.cigar_string = None

    def _cigar_string(self, cigar, query_len):
        """BAM-style u32 ops -> SAM text, soft clips added at both ends (ssw_wrap.py:349-379)."""
        parts = []
        if self.query_begin > 0:
            parts.append('%dS' % self.query_begin)
        for c in cigar:
            c = int(c)
            code = c & 0xf
            parts.append('%d%s' % (c >> 4, _OPS[code] if code < len(_OPS) else 'M'))
        tail = query_len - self.query_end - 1
        if tail != 0:
            parts.append('%dS' % tail)
        return ''.join(parts)

    def __str__(self):
        return "\n<Instance of {} from {} >\n".format(self.__class__.__name__, self.__module__)

    def __repr__(self):
        msg = self.__str__()
        msg += "OPTIMAL MATCH\n"
        msg += "Score            {}\n".format(self.score)
        msg += "Reference begin  {}\n".format(self.ref_begin)
        msg += "Reference end    {}\n".format(self.ref_end)
        msg += "Query begin      {}\n".format(self.query_begin)
        msg += "Query end        {}\n".format(self.query_end)
        if self.cigar_string:
            msg += "Cigar_string     {}\n".format(self.cigar_string)
        if self.score2:
            msg += "SUB-OPTIMAL MATCH\n"
            msg += "Score 2           {}\n".format(self.score2)
            msg += "Ref_end2          {}\n".format(self.ref_end2)
        return msg


def _filter(row, cig, query_len, min_score, min_len, report_secondary, report_cigar):
    """Everything after the FFI call in ssw_wrap.py:211-222."""
    if int(row['status']) & (hip.ST_NULL | hip.ST_TRACE_ERR | hip.ST_CIGAR_TRUNC):
        return None            # the reference's NULL result: score := -999999999999 -> filtered out
    res = CAlignRes(row, cig)
    if res.score >= min_score and (res.query_end - res.query_begin + 1) >= min_len:
        return PyAlignRes(res, query_len, report_secondary, report_cigar)
    return None


def align_pairs(ref_seqs, query_seqs, match=2, mismatch=2, gap_open=3, gap_extend=1, report_secondary=False,
                report_cigar=False, min_score=0, min_len=0, context=None):
    """n independent (reference, query) alignments in one GPU call; element k equals
    ``Aligner(ref_seqs[k], ...).align(query_seqs[k], min_score, min_len)``.  Sequences are ``str`` or int8 code arrays."""
    if len(ref_seqs) != len(query_seqs):
        raise ValueError('align_pairs: %d references vs %d queries' % (len(ref_seqs), len(query_seqs)))
    if not ref_seqs:
        return []
    ctx = context or hip.default_context()
    qd, qo = hip.pack(query_seqs)
    rd, ro = hip.pack(ref_seqs)
    rows, cig = ctx.ssw_batch(qd, qo, rd, ro, hip.score_matrix(match, mismatch), gap_open, gap_extend, flag=1, score_size=2,
                              want_score2=bool(report_secondary), want_cigar=bool(report_cigar))
    out = []
    for k in range(len(rows)):
        r = rows[k]
        c = cig[r['cigar_off']:r['cigar_off'] + r['cigar_len']] if r['cigar_len'] > 0 else ()
        out.append(_filter(r, c, int(qo[k + 1] - qo[k]), min_score, min_len, report_secondary, report_cigar))
    return out


def align_windows(genome, windows, minus, query_seqs, match=2, mismatch=2, gap_open=3, gap_extend=1, report_secondary=False,
                  report_cigar=False, min_score=0, min_len=0):
    """align_pairs with reference k = window (contig, start, end) of a genome resident on the GPU (hip.Genome),
    reverse-complemented the reference's way where minus[k]: element k equals
    ``Aligner(revcomp(seq) if minus[k] else seq, ...).align(query_seqs[k])`` for seq = the window's string."""
    if len(windows) != len(query_seqs):
        raise ValueError('align_windows: %d windows vs %d queries' % (len(windows), len(query_seqs)))
    if not windows:
        return []
    qd, qo = hip.pack(query_seqs)
    rows, cig = genome.ssw_windows(qd, qo, windows, minus, hip.score_matrix(match, mismatch), gap_open, gap_extend, flag=1, score_size=2,
                                   want_score2=bool(report_secondary), want_cigar=bool(report_cigar))
    out = []
    for k in range(len(rows)):
        r = rows[k]
        c = cig[r['cigar_off']:r['cigar_off'] + r['cigar_len']] if r['cigar_len'] > 0 else ()
        out.append(_filter(r, c, int(qo[k + 1] - qo[k]), min_score, min_len, report_secondary, report_cigar))
    return out


class Aligner(object):
    """One reference sequence, many queries (ssw_wrap.py:40-264)."""

    base_to_int = {'A': 0, 'C': 1, 'G': 2, 'T': 3, 'N': 4, 'a': 0, 'c': 1, 'g': 2, 't': 3, 'n': 4}
    int_to_base = {0: 'A', 1: 'C', 2: 'G', 3: 'T', 4: 'N'}

    def __init__(self, ref_seq="", match=2, mismatch=2, gap_open=3, gap_extend=1, report_secondary=False,
                 report_cigar=False, context=None):
        self.report_secondary = report_secondary
        self.report_cigar = report_cigar
        self._context = context
        self.set_gap(gap_open, gap_extend)
        self.set_mat(match, mismatch)
        self.set_ref(ref_seq)

    # -- setters, ssw_wrap.py:137-170 --
    def set_gap(self, gap_open=3, gap_extend=1):
        self.gap_open = gap_open
        self.gap_extend = gap_extend

    def set_mat(self, match=2, mismatch=2):
        self.match = match
        self.mismatch = mismatch
        self.mat = hip.score_matrix(match, mismatch)

    def set_ref(self, ref_seq):
        if ref_seq is not None and len(ref_seq):
            self.ref_seq = self._DNA_to_int_mat(ref_seq, len(ref_seq))
            self.ref_len = len(self.ref_seq)
        else:
            self.ref_len = 0
            self.ref_seq = ""

    def _DNA_to_int_mat(self, seq, len_seq):
        if isinstance(seq, np.ndarray):
            return np.ascontiguousarray(seq[:len_seq], dtype=np.int8)
        return hip.encode(seq[:len_seq])

    # -- alignment --
    def align(self, query_seq, min_score=0, min_len=0):
        res = self.align_batch([query_seq], min_score, min_len)
        return res[0]

    def align_batch(self, query_seqs, min_score=0, min_len=0):
        """All queries against this reference in one GPU call; element k equals ``self.align(query_seqs[k], ...)``."""
        n = len(query_seqs)
        if n == 0:
            return []
        if self.ref_len == 0:
            raise ValueError('Aligner has no reference sequence')
        ctx = self._context or hip.default_context()
        qd, qo = hip.pack([self._DNA_to_int_mat(q, len(q)) for q in query_seqs])
        rd = np.tile(self.ref_seq, n) if n > 1 else self.ref_seq
        ro = np.arange(n + 1, dtype=np.int64) * self.ref_len
        rows, cig = ctx.ssw_batch(qd, qo, rd, ro, self.mat, self.gap_open, self.gap_extend, flag=1, score_size=2,
                                  want_score2=bool(self.report_secondary), want_cigar=bool(self.report_cigar))
        out = []
        for k in range(n):
            r = rows[k]
            c = cig[r['cigar_off']:r['cigar_off'] + r['cigar_len']] if r['cigar_len'] > 0 else ()
            out.append(_filter(r, c, int(qo[k + 1] - qo[k]), min_score, min_len, self.report_secondary, self.report_cigar))
        return out

    def __str__(self):
        return "\n<Instance of {} from {} >\n".format(self.__class__.__name__, self.__module__)

    def __repr__(self):
        msg = self.__str__()
        msg += "SCORE PARAMETERS:\n"
        msg += " Gap Weight     Open: {}     Extension: {}\n".format(-self.gap_open, -self.gap_extend)
        msg += " Align Weight   Match: {}    Mismatch: {}\n\n".format(self.match, -self.mismatch)
        msg += "RESULT PARAMETERS:\n"
        msg += " Report cigar           {}\n".format(self.report_cigar)
        msg += " Report secondary match {}\n\n".format(self.report_secondary)
        msg += "REFERENCE SEQUENCE :\n"
        shown = min(self.ref_len, 50)
        msg += "".join(self.int_to_base[int(self.ref_seq[i])] for i in range(shown)) + ("...\n" if self.ref_len > 50 else "\n")
        msg += " Lenght :{} nucleotides\n".format(self.ref_len)
        return msg


# ---------------------------------------------------------------------------------------------------------------------------
# alphabets of up to 32 letters (ssw_init takes an n x n matrix for any n; libclh.so up to n = 32)
# ---------------------------------------------------------------------------------------------------------------------------
BLOSUM62_ALPHABET = 'ARNDCQEGHILKMFPSTWYVBZX*'
# the published NCBI BLOSUM62 table, rows and columns in BLOSUM62_ALPHABET order
_BLOSUM62_ROWS = """
 4 -1 -2 -2  0 -1 -1  0 -2 -1 -1 -1 -1 -2 -1  1  0 -3 -2  0 -2 -1  0 -4
-1  5  0 -2 -3  1  0 -2  0 -3 -2  2 -1 -3 -2 -1 -1 -3 -2 -3 -1  0 -1 -4
-2  0  6  1 -3  0  0  0  1 -3 -3  0 -2 -3 -2  1  0 -4 -2 -3  3  0 -1 -4
-2 -2  1  6 -3  0  2 -1 -1 -3 -4 -1 -3 -3 -1  0 -1 -4 -3 -3  4  1 -1 -4
 0 -3 -3 -3  9 -3 -4 -3 -3 -1 -1 -3 -1 -2 -3 -1 -1 -2 -2 -1 -3 -3 -2 -4
-1  1  0  0 -3  5  2 -2  0 -3 -2  1  0 -3 -1  0 -1 -2 -1 -2  0  3 -1 -4
-1  0  0  2 -4  2  5 -2  0 -3 -3  1 -2 -3 -1  0 -1 -3 -2 -2  1  4 -1 -4
 0 -2  0 -1 -3 -2 -2  6 -2 -4 -4 -2 -3 -3 -2  0 -2 -2 -3 -3 -1 -2 -1 -4
-2  0  1 -1 -3  0  0 -2  8 -3 -3 -1 -2 -1 -2 -1 -2 -2  2 -3  0  0 -1 -4
-1 -3 -3 -3 -1 -3 -3 -4 -3  4  2 -3  1  0 -3 -2 -1 -3 -1  3 -3 -3 -1 -4
-1 -2 -3 -4 -1 -2 -3 -4 -3  2  4 -2  2  0 -3 -2 -1 -2 -1  1 -4 -3 -1 -4
-1  2  0 -1 -3  1  1 -2 -1 -3 -2  5 -1 -3 -1  0 -1 -3 -2 -2  0  1 -1 -4
-1 -1 -2 -3 -1  0 -2 -3 -2  1  2 -1  5  0 -2 -1 -1 -1 -1  1 -3 -1 -1 -4
-2 -3 -3 -3 -2 -3 -3 -3 -1  0  0 -3  0  6 -4 -2 -2  1  3 -1 -3 -3 -1 -4
-1 -2 -2 -1 -3 -1 -1 -2 -2 -3 -3 -1 -2 -4  7 -1 -1 -4 -3 -2 -2 -1 -2 -4
 1 -1  1  0 -1  0  0  0 -1 -2 -2  0 -1 -2 -1  4  1 -3 -2 -2  0  0  0 -4
 0 -1  0 -1 -1 -1 -1 -2 -2 -1 -1 -1 -1 -2 -1  1  5 -2 -2  0 -1 -1  0 -4
-3 -3 -4 -4 -2 -2 -3 -2 -2 -3 -2 -3 -1  1 -4 -3 -2 11  2 -3 -4 -3 -2 -4
-2 -2 -2 -3 -2 -1 -2 -3  2 -1 -1 -2 -1  3 -3 -2 -2  2  7 -1 -3 -2 -1 -4
 0 -3 -3 -3 -1 -2 -2 -3 -3  3  1 -2  1 -1 -2 -2  0 -3 -1  4 -3 -2 -1 -4
-2 -1  3  4 -3  0  1 -1  0 -3 -4  0 -3 -3 -2  0 -1 -4 -3 -3  4  1 -1 -4
-1  0  0  1 -3  3  4 -2  0 -3 -3  1 -1 -3 -1  0 -1 -3 -2 -2  1  4 -1 -4
 0 -1 -1 -1 -2 -1 -1 -1 -1 -1 -1 -1 -1 -1 -2  0  0 -2 -1 -1 -1 -1 -1 -4
-4 -4 -4 -4 -4 -4 -4 -4 -4 -4 -4 -4 -4 -4 -4 -4 -4 -4 -4 -4 -4 -4 -4  1
"""
BLOSUM62 = np.array([int(x) for x in _BLOSUM62_ROWS.split()], dtype=np.int8).reshape(24, 24)


def encode_alphabet(seq, alphabet, unknown=None):
    """str / bytes -> int8 codes: the index of each letter in `alphabet`, upper and lower case alike.  A letter outside the
    alphabet raises ValueError, unless `unknown` names a letter of the alphabet to stand for it."""
    if len(alphabet) > 32 or len(alphabet) < 1:
        raise ValueError('encode_alphabet: alphabets of 1..32 letters')
    lut = np.full(256, -1, dtype=np.int16)
    for i, ch in enumerate(alphabet):
        for c in {ch.upper(), ch.lower()}:
            if lut[ord(c)] < 0:
                lut[ord(c)] = i
    if isinstance(seq, str):
        seq = seq.encode('latin-1')
    codes = lut[np.frombuffer(bytes(seq), dtype=np.uint8)]
    if codes.size and codes.min() < 0:
        if unknown is None:
            bad = bytes(seq)[int(np.argmax(codes < 0))]
            raise ValueError('encode_alphabet: letter %r is not in the alphabet' % chr(bad))
        k = alphabet.find(unknown) if len(unknown) == 1 else -1
        if k < 0:
            k = alphabet.upper().find(unknown.upper()) if len(unknown) == 1 else -1
        if k < 0:
            raise ValueError('encode_alphabet: unknown=%r is not a letter of the alphabet' % (unknown,))
        codes = np.where(codes < 0, k, codes)
    return np.ascontiguousarray(codes, dtype=np.int8)


def _int8_matrix(matrix, who):
    """a substitution matrix as flat int8; an entry the kernels' int8 cannot hold raises and is named, it does not wrap"""
    mat = np.asarray(matrix)
    if mat.dtype != np.int8 and mat.size:
        bad = np.argwhere(~((mat >= -128) & (mat <= 127)))
        if len(bad):
            at = tuple(int(x) for x in bad[0])
            raise ValueError('%s: matrix%s = %s is outside -128..127, the range of a score' % (who, ''.join('[%d]' % x for x in at), mat[at]))
    return np.ascontiguousarray(mat, dtype=np.int8).reshape(-1)


def align_pairs_matrix(ref_seqs, query_seqs, matrix, alphabet, gap_open, gap_extend, report_secondary=False,
                       report_cigar=False, min_score=0, min_len=0, context=None):
    """align_pairs over an alphabet of up to 32 letters: element k is what the reference's ssw_init(query k, matrix) +
    ssw_align(reference k, gap_open, gap_extend, flag 1) + its Python wrapper's filter would give, as a PyAlignRes or None.
    matrix: n x n (row = reference letter), n = len(alphabet); sequences are str (letters of `alphabet`, any case) or
    int8 code arrays."""
    if len(ref_seqs) != len(query_seqs):
        raise ValueError('align_pairs_matrix: %d references vs %d queries' % (len(ref_seqs), len(query_seqs)))
    mat = _int8_matrix(matrix, 'align_pairs_matrix')
    n = len(alphabet)
    if mat.size != n * n:
        raise ValueError('align_pairs_matrix: a %d-letter alphabet needs a %d x %d matrix' % (n, n, n))
    if not ref_seqs:
        return []
    enc = lambda s: encode_alphabet(s, alphabet) if isinstance(s, (str, bytes)) else np.asarray(s, dtype=np.int8)
    qd, qo = hip.pack([enc(q) for q in query_seqs])
    rd, ro = hip.pack([enc(r) for r in ref_seqs])
    ctx = context or hip.default_context()
    rows, cig = ctx.ssw_batch(qd, qo, rd, ro, mat, gap_open, gap_extend, flag=1, score_size=2,
                              want_score2=bool(report_secondary), want_cigar=bool(report_cigar))
    out = []
    for k in range(len(rows)):
        r = rows[k]
        c = cig[r['cigar_off']:r['cigar_off'] + r['cigar_len']] if r['cigar_len'] > 0 else ()
        out.append(_filter(r, c, int(qo[k + 1] - qo[k]), min_score, min_len, report_secondary, report_cigar))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# end-anchored modes beside the local one (K1g, csrc/ssw_ends.hip)
# ---------------------------------------------------------------------------------------------------------------------------
def _pairs_inputs(who, ref_seqs, query_seqs, match, mismatch, matrix, alphabet):
    """what align_pairs_ends and align_pairs_band send to the device: the flat int8 matrix (match / mismatch, or `matrix` over
    `alphabet`), and the packed codes (data, offsets) of the queries and of the references"""
    if (matrix is None) != (alphabet is None):
        raise ValueError('%s: matrix and alphabet come together' % who)
    if matrix is not None:
        mat = _int8_matrix(matrix, who)
        if mat.size != len(alphabet) ** 2 or not 1 <= len(alphabet) <= 32:
            raise ValueError('%s: a %d-letter alphabet needs a %d x %d matrix (1..32 letters)' % (who, len(alphabet), len(alphabet), len(alphabet)))
        enc = lambda s: encode_alphabet(s, alphabet) if isinstance(s, (str, bytes)) else np.asarray(s, dtype=np.int8)
    else:
        mat = hip.score_matrix(match, mismatch)
        enc = lambda s: hip.encode(s) if isinstance(s, (str, bytes)) else np.asarray(s, dtype=np.int8)
    return mat, hip.pack([enc(q) for q in query_seqs]), hip.pack([enc(r) for r in ref_seqs])


def _pairs_results(rows, cig, qo, walk, report_cigar):
    """rows of ENDS_DTYPE's fields and their CIGAR ops -> one PyAlignRes per pair"""
    out = []
    for k in range(len(rows)):
        r = rows[k]
        ops = cig[int(r['cigar_off']):int(r['cigar_off']) + int(r['cigar_len'])] if walk else ()
        res = PyAlignRes.__new__(PyAlignRes)
        res.score = int(r['score'])
        res.ref_begin, res.ref_end = int(r['ref_begin']), int(r['ref_end'])
        res.query_begin, res.query_end = int(r['query_begin']), int(r['query_end'])
        res.score2 = res.ref_end2 = None
        res.cigar_string = res._cigar_string(ops, int(qo[k + 1] - qo[k])) if report_cigar else None
        out.append(res)
    return out


# the two-piece gap costs of the long-read presets (-O4,24 -E2,1 at 2 / 4): keywords for align_pairs_ends, align_pairs_band and extend_anchors.  A
# convenience; nothing is claimed about parity with any other aligner's output.
LONG_READ_GAPS = dict(match=2, mismatch=4, gap_open=4, gap_extend=2, gap_open2=24, gap_extend2=1)


def align_pairs_ends(ref_seqs, query_seqs, mode='global', match=2, mismatch=2, gap_open=3, gap_extend=1, report_cigar=False, matrix=None,
                     alphabet=None, context=None, gap_open2=None, gap_extend2=None, traceback='stored'):
    """n independent (reference, query) alignments anchored at the ends, in one GPU call -> one PyAlignRes per pair.

    mode 'global': both sequences end to end.  'semiglobal': the whole query in any stretch of the reference (a probe, an exon, a
    junction placed inside a read).  'overlap': end gaps free on both sequences at both ends (dovetails, containment).
    'prefix' and 'extend' are anchored at the start, (0, 0), and free at the far end: 'prefix' aligns the whole query against a
    prefix of the reference (the best cell of the last row, smallest column; at match 0 and unit costs the score is minus edlib's SHW
    distance), 'extend' a prefix of the query against a prefix of the reference (the best cell of the whole matrix, (0, 0) with
    score 0 included, smallest query row, then smallest reference column; the score is >= 0 and the empty result has ref_end =
    query_end = -1).  Both are defined by the full matrix, not by a z-drop or X-drop rule; ``extend_anchors`` uses 'extend'.  Scores are
    those of ``align_pairs`` -- match / mismatch, or `matrix` (n x n, row = reference letter) over `alphabet` as in
    ``align_pairs_matrix`` -- with a gap of k letters costing gap_open + (k - 1) gap_extend, gap_open >= gap_extend.

    ``score`` may be negative.  Coordinates are 0-based and inclusive; a span that consumed no letter has end == begin - 1.  Ties: the
    semiglobal end is the smallest reference column with the best score; the overlap end is sought in the last row first (smallest
    column), then in the last column (smallest row); the walk back prefers the diagonal, then a reference letter against nothing
    (D), then a query letter against nothing (I), and leaves a gap as soon as it can.  ``score2`` and ``ref_end2`` are None.
    ``cigar_string`` (report_cigar) uses M / I / D, with soft clips for the query letters outside query_begin..query_end as
    ``align_pairs`` writes them.  Parity with other libraries' tie rules is not pinned.

    gap_open2 and gap_extend2 (together) add a second piece: a gap of k letters then costs the smaller of gap_open + (k - 1)
    gap_extend and gap_open2 + (k - 1) gap_extend2, piece 1 for short gaps and piece 2 for long ones, 0 <= gap_extend2 <=
    gap_extend <= gap_open <= gap_open2 (``LONG_READ_GAPS`` is such a set).  The walk back then prefers the diagonal, D by piece 1,
    D by piece 2, I by piece 1, I by piece 2; the CIGAR does not say which piece paid.

    traceback: 'stored' keeps the decisions of every cell of a pair on the device for the walk back; 'recompute' keeps one column per
    512 reference columns and computes the decisions again chunk by chunk -- the same results from a fraction of the memory, for
    pairs whose reference is thousands of letters long (``hip.EndsPlan``)."""
    two = {} if hip.gap2_of('align_pairs_ends', gap_open2, gap_extend2) is None else dict(gap_open2=gap_open2, gap_extend2=gap_extend2)
    if traceback not in hip.ENDS_TRACEBACKS:
        raise ValueError("align_pairs_ends: traceback must be 'stored' or 'recompute', got %r" % (traceback,))
    if traceback != 'stored':
        two = dict(two, traceback=traceback)
    if mode not in hip.ENDS_MODES:
        raise ValueError("align_pairs_ends: mode must be 'global', 'semiglobal', 'overlap', 'prefix' or 'extend', got %r" % (mode,))
    if len(ref_seqs) != len(query_seqs):
        raise ValueError('align_pairs_ends: %d references vs %d queries' % (len(ref_seqs), len(query_seqs)))
    mat, (qd, qo), (rd, ro) = _pairs_inputs('align_pairs_ends', ref_seqs, query_seqs, match, mismatch, matrix, alphabet)
    if not ref_seqs:
        return []
    ctx = context or hip.default_context()
    walk = bool(report_cigar) or mode in ('semiglobal', 'overlap')      # the begins come from the walk, unless the mode fixes them
    rows, cig = ctx.ends_batch(qd, qo, rd, ro, mat, gap_open, gap_extend, mode=mode, want_cigar=walk, **two)      # one piece: the call as it always was
    return _pairs_results(rows, cig, qo, walk, report_cigar)


# the defaults of align_pairs_spliced as keywords: match 2, mismatch 2, a deletion 3 + 1 per further letter, an intron 12 between GT and
# AG and 6 more per site that is not canonical.  A convenience; nothing is claimed about parity with any other aligner's output.
SPLICED_DEFAULTS = dict(match=2, mismatch=2, gap_open=3, gap_extend=1, intron_open=12, noncanonical=6)


def _strands(strand, n):
    """'+', '-', +1, -1 or a sequence of them -> int8[n] of +1 / -1"""
    one = {'+': 1, '-': -1, 1: 1, -1: -1}
    if isinstance(strand, (str, bytes, int, np.integer)):
        strand = [strand] * n
    strand = list(strand)
    if len(strand) != n or any((s.decode() if isinstance(s, bytes) else s) not in one for s in strand):
        raise ValueError("align_pairs_spliced: strand must be '+', '-', 'both' or one of '+' / '-' per pair, got %r" % (strand[:8],))
    return np.array([one[s.decode() if isinstance(s, bytes) else s] for s in strand], dtype=np.int8)


def align_pairs_spliced(ref_seqs, query_seqs, mode='semiglobal', strand='+', match=2, mismatch=2, gap_open=3, gap_extend=1, intron_open=12, noncanonical=6,
                        donor_costs=None, acceptor_costs=None, report_cigar=False, context=None, matrix=None, alphabet=None, gap_open2=None,
                        gap_extend2=None, traceback='stored'):
    """``align_pairs_ends`` of a transcript sequence (query) against a genomic window (reference) in which a long reference gap may be an
    intron, in one GPU call -> one PyAlignRes per pair, each with ``.strand`` ('+' or '-').

    A maximal run of skipped reference letters r[a..b] costs the smaller of gap_open + (b - a) gap_extend and intron_open + start(a) +
    end(b): an intron costs a constant whatever its length.  On strand '+', start(a) is the donor cost of the dinucleotide r[a] r[a+1]
    and end(b) the acceptor cost of r[b-1] r[b]; on strand '-' the transcript is the reverse complement, so the acceptor cost of the
    complement of r[a+1] r[a] opens and the donor cost of the complement of r[b] r[b-1] closes (a canonical intron reads CT..AC).  GT
    as donor and AG as acceptor cost 0; every other dinucleotide, and one that holds an N or runs off the window, costs `noncanonical`;
    donor_costs / acceptor_costs override single dinucleotides as read on the transcript strand, e.g. donor_costs={'GC': 2}.  The costs
    depend on the position alone.  A deletion and an intron are never adjacent; insertions are as in ``align_pairs_ends``, as are the
    modes, end cells, coordinates and ties (csrc/ssw_ends.hip; tests/spliced_check.py is the definition).

    strand is '+', '-', a sequence of them (one per pair), or 'both': every pair is then aligned on both strands in the same call and
    the higher score is kept, ties to '+'.  ``cigar_string`` (report_cigar) uses M / I / D / N with soft clips as ``align_pairs_ends``
    writes them, which ``align.convert_cigar_string`` and ``align.get_exons`` read; among equal scores the walk prefers the diagonal,
    then D, then N, then I, and a run on row 0 of an anchored mode is D unless N is cheaper.  DNA match / mismatch only: `matrix`,
    `alphabet`, `gap_open2` and `gap_extend2` are named here to be refused (not built).  All costs are >= 0 and gap_open >=
    gap_extend.  Parity with minimap2's splice model, which couples donor and acceptor and has other tie rules, is not claimed.
    traceback is ``align_pairs_ends``'s: 'recompute' is the route for a cDNA against a gene locus of tens of kilobases."""
    who = 'align_pairs_spliced'
    if traceback not in hip.ENDS_TRACEBACKS:
        raise ValueError("%s: traceback must be 'stored' or 'recompute', got %r" % (who, traceback))
    if matrix is not None or alphabet is not None:
        raise ValueError('%s: substitution matrices are not supported (CLH_E_UNSUPPORTED): DNA match / mismatch only' % who)
    if gap_open2 is not None or gap_extend2 is not None:
        raise ValueError('%s: two-piece gap costs together with introns are not supported (CLH_E_UNSUPPORTED)' % who)
    if mode not in hip.ENDS_MODES:
        raise ValueError("%s: mode must be 'global', 'semiglobal', 'overlap', 'prefix' or 'extend', got %r" % (who, mode))
    n = len(ref_seqs)
    if len(query_seqs) != n:
        raise ValueError('%s: %d references vs %d queries' % (who, n, len(query_seqs)))
    if min(int(match), int(mismatch), int(gap_open), int(gap_extend)) < 0:
        raise ValueError('%s: match, mismatch and the gap costs must not be negative' % who)
    splice = hip.splice_of(who, intron_open, noncanonical, donor_costs, acceptor_costs)
    both = isinstance(strand, str) and strand == 'both'
    st = np.concatenate([np.ones(n, dtype=np.int8), -np.ones(n, dtype=np.int8)]) if both else _strands(strand, n)
    if not n:
        return []
    refs, queries = (list(ref_seqs) * 2, list(query_seqs) * 2) if both else (ref_seqs, query_seqs)      # 'both': pair k and pair n + k, one plan
    mat, (qd, qo), (rd, ro) = _pairs_inputs(who, refs, queries, match, mismatch, None, None)
    ctx = context or hip.default_context()
    walk = bool(report_cigar) or mode in ('semiglobal', 'overlap')      # the begins come from the walk, unless the mode fixes them
    route = {} if traceback == 'stored' else dict(traceback=traceback)
    rows, cig = ctx.ends_batch(qd, qo, rd, ro, mat, gap_open, gap_extend, mode=mode, want_cigar=walk, splice=splice, strand=st, **route)
    out = _pairs_results(rows, cig, qo, walk, report_cigar)
    for res, s in zip(out, st):
        res.strand = '+' if s > 0 else '-'
    if both:
        out = [out[k] if out[k].score >= out[n + k].score else out[n + k] for k in range(n)]
    return out


def align_pairs_band(ref_seqs, query_seqs, band, mode='global', diagonals=None, match=2, mismatch=2, gap_open=3, gap_extend=1, report_cigar=False,
                     matrix=None, alphabet=None, context=None, gap_open2=None, gap_extend2=None):
    """``align_pairs_ends`` over a band of diagonals, in one GPU call -> one PyAlignRes per pair.

    With i query and j reference letters consumed, only cells with lo <= j - i <= hi exist: lo = min(0, n - m) - band and hi =
    max(0, n - m) + band (the corner diagonals of the m x n pair widened by `band`), or diagonals[k] - band and diagonals[k] + band
    where a placement is known (a seed, a minimizer hit, an ``edlib.search`` location: the diagonal is reference position minus
    query position); both clipped to [-m, n], at most 512 diagonals.  mode is 'global', 'semiglobal', 'prefix' or 'extend'; for the
    last two, whose far end is free, the band without a hint is [-band, band], it must hold diagonal 0, and end cells are taken over
    the band's cells only.  Scores, coordinates, tie rules and the CIGAR are those of ``align_pairs_ends``, and every result is the
    best alignment that stays inside the band.  Each
    result also carries ``band`` = (lo, hi) as clipped, and ``band_exact``: True where it is proved that ``align_pairs_ends`` returns
    the same result and CIGAR (False: not proved; they may still be equal).  The cost is m x (hi - lo + 1) cells, not m x n, and
    CIGARs need half a byte per cell of the band.  A band that holds no alignment, 'overlap', and a band above 512 diagonals raise
    hip.ClhError.  gap_open2 and gap_extend2 are the two-piece gap costs of ``align_pairs_ends``; CIGARs then
    need a byte per cell of the band, and ``band_exact`` is the same certificate with a run costed by the cheaper piece."""
    two = {} if hip.gap2_of('align_pairs_band', gap_open2, gap_extend2) is None else dict(gap_open2=gap_open2, gap_extend2=gap_extend2)
    if mode not in ('global', 'semiglobal', 'prefix', 'extend'):
        raise ValueError("align_pairs_band: mode must be 'global', 'semiglobal', 'prefix' or 'extend'%s, got %r"
                         % (" ('overlap' with a band is not built)" if mode == 'overlap' else '', mode))
    if len(ref_seqs) != len(query_seqs):
        raise ValueError('align_pairs_band: %d references vs %d queries' % (len(ref_seqs), len(query_seqs)))
    if diagonals is not None and len(diagonals) != len(ref_seqs):
        raise ValueError('align_pairs_band: %d diagonals vs %d pairs' % (len(diagonals), len(ref_seqs)))
    if int(band) != band or band < 0:
        raise ValueError('align_pairs_band: band is a half-width in diagonals, an integer >= 0, got %r' % (band,))
    mat, (qd, qo), (rd, ro) = _pairs_inputs('align_pairs_band', ref_seqs, query_seqs, match, mismatch, matrix, alphabet)
    if not ref_seqs:
        return []
    ctx = context or hip.default_context()
    walk = bool(report_cigar) or mode == 'semiglobal'      # the begins come from the walk, unless the mode fixes them
    rows, cig = ctx.band_batch(qd, qo, rd, ro, mat, gap_open, gap_extend, int(band), mode=mode, diagonals=diagonals, want_cigar=walk, **two)
    out = _pairs_results(rows, cig, qo, walk, report_cigar)
    for r, res in zip(rows, out):
        res.band = (int(r['band_lo']), int(r['band_hi']))
        res.band_exact = bool(r['exact'])
    return out


def _merge_ops(ops):
    """(op, length) runs with equal neighbours merged"""
    out = []
    for op, k in ops:
        if k <= 0:
            continue
        if out and out[-1][0] == op:
            out[-1] = (op, out[-1][1] + k)
        else:
            out.append((op, k))
    return out


def _stitch_anchor(left, right, ref_pos, query_pos, seed_len, seed_score=0):
    """one result of extend_anchors from the 'extend' rows of its two halves: `left` of the reversed letters before the anchor,
    `right` of the letters after it (and after the seed); each half is (score, ref_end, query_end, ops) in its own coordinates"""
    ls, lre, lqe, lops = left
    rs, rre, rqe, rops = right
    ops = _merge_ops(list(reversed(lops)) + [('M', seed_len)] + list(rops))
    return (ls + seed_score + rs, ref_pos - (lre + 1), ref_pos + seed_len + rre, query_pos - (lqe + 1), query_pos + seed_len + rqe, ops)


def extend_anchors(ref_seqs, query_seqs, anchors, band=None, seed_len=0, match=2, mismatch=2, gap_open=3, gap_extend=1, report_cigar=False,
                   matrix=None, alphabet=None, context=None, gap_open2=None, gap_extend2=None, traceback='stored'):
    """Extend n placements both ways, in one GPU call -> one PyAlignRes per pair.

    anchors[k] = (ref_pos, query_pos) is a point between letters of pair k: what an ``edlib.search`` location, a minimizer hit or
    an exact seed gives.  The right part is mode 'extend' of ``align_pairs_ends`` on ref[ref_pos:] against query[query_pos:]; the
    left part is 'extend' on the reversed ref[:ref_pos] against the reversed query[:query_pos].  With seed_len > 0 the anchor is
    the first letter of an exact seed of that many letters in both sequences: the left part ends in front of it, the right part
    starts behind it, and seed_len M columns with their score under the matrix stand between the halves.  Both parts
    of all pairs go to the device as one plan of 2 n pairs: K1g if band is None, else K1gb with the band [-band, band] around
    each half's own diagonal 0.

    Result: ``score`` is the sum of both parts (each >= 0) and of the seed's columns; begins and ends are in the coordinates of the sequences as given, inclusive,
    end == begin - 1 where nothing was consumed; ``cigar_string`` (report_cigar) is the left part's ops reversed, the seed, the
    right part's ops, equal neighbours merged, with soft clips for the query letters outside.  With a band, ``band_exact`` is True
    only where both halves are proved equal to the unbanded result.  The left half is aligned on reversed letters, so among equal
    scores its ties (the end cell, and diagonal before D before I in the walk) are those of the reversed problem: it is the best
    extension to the left, but not necessarily the one a single left-to-right programme over the joined sequences would pick.
    gap_open2 and gap_extend2 are those of ``align_pairs_ends`` and ``align_pairs_band`` (two-piece gap costs); traceback is that of
    ``align_pairs_ends`` and goes with band=None alone: the band's planes are already m x B."""
    two = {} if hip.gap2_of('extend_anchors', gap_open2, gap_extend2) is None else dict(gap_open2=gap_open2, gap_extend2=gap_extend2)
    if traceback not in hip.ENDS_TRACEBACKS:
        raise ValueError("extend_anchors: traceback must be 'stored' or 'recompute', got %r" % (traceback,))
    if traceback != 'stored' and band is not None:
        raise ValueError("extend_anchors: traceback=%r goes with band=None: K1gb has the stored route alone" % (traceback,))
    n = len(ref_seqs)
    if len(query_seqs) != n or len(anchors) != n:
        raise ValueError('extend_anchors: %d references vs %d queries vs %d anchors' % (n, len(query_seqs), len(anchors)))
    if int(seed_len) != seed_len or seed_len < 0:
        raise ValueError('extend_anchors: seed_len is a number of letters >= 0, got %r' % (seed_len,))
    if band is not None and (int(band) != band or band < 0):
        raise ValueError('extend_anchors: band is a half-width in diagonals, an integer >= 0, got %r' % (band,))
    seed_len = int(seed_len)
    refs2, queries2 = [], []
    for k in range(n):
        rp, qp = int(anchors[k][0]), int(anchors[k][1])
        r, q = ref_seqs[k], query_seqs[k]
        if not (0 <= rp and rp + seed_len <= len(r) and 0 <= qp and qp + seed_len <= len(q)):
            raise ValueError('extend_anchors: pair %d: the anchor (%d, %d) with seed_len %d lies outside the %d x %d pair'
                             % (k, rp, qp, seed_len, len(q), len(r)))
        refs2.append(r[:rp][::-1]); queries2.append(q[:qp][::-1])
        refs2.append(r[rp + seed_len:]); queries2.append(q[qp + seed_len:])
    if not n:
        return []
    seed_scores = [0] * n
    if seed_len:
        mat, (qd, qo), (rd, ro) = _pairs_inputs('extend_anchors', [ref_seqs[k][anchors[k][0]:anchors[k][0] + seed_len] for k in range(n)],
                                                [query_seqs[k][anchors[k][1]:anchors[k][1] + seed_len] for k in range(n)], match, mismatch, matrix, alphabet)
        edge = int(round(mat.size ** 0.5))
        cols = np.asarray(mat, dtype=np.int64).reshape(edge, edge)[np.asarray(rd, dtype=np.int64), np.asarray(qd, dtype=np.int64)]
        seed_scores = [int(cols[k * seed_len:(k + 1) * seed_len].sum()) for k in range(n)]
    kw = dict(mode='extend', match=match, mismatch=mismatch, gap_open=gap_open, gap_extend=gap_extend, report_cigar=bool(report_cigar),
              matrix=matrix, alphabet=alphabet, context=context)
    kw.update(two)
    if traceback != 'stored':
        kw['traceback'] = traceback
    halves = align_pairs_ends(refs2, queries2, **kw) if band is None else align_pairs_band(refs2, queries2, int(band), **kw)
    return _stitch_halves(halves, [(int(a[0]), int(a[1])) for a in anchors], [len(q) for q in query_seqs], seed_len, seed_scores, report_cigar, band is not None)


def _stitch_halves(halves, anchors, query_lens, seed_len, seed_scores, report_cigar, banded):
    """the results of extend_anchors from the 'extend' results of its 2 n halves (left of pair k at 2 k, right at 2 k + 1);
    anchors[k] = (ref_pos, query_pos)"""
    n = len(anchors)
    out = []
    for k in range(n):
        parts = []
        for h in (halves[2 * k], halves[2 * k + 1]):
            ops = []
            if report_cigar:
                num = ''
                for ch in h.cigar_string or '':
                    if ch.isdigit():
                        num += ch
                    else:
                        if ch != 'S':
                            ops.append((ch, int(num)))
                        num = ''
            parts.append((h.score, h.ref_end, h.query_end, ops))
        score, rb, re_, qb, qe, ops = _stitch_anchor(parts[0], parts[1], anchors[k][0], anchors[k][1], seed_len, seed_scores[k])
        res = PyAlignRes.__new__(PyAlignRes)
        res.score, res.ref_begin, res.ref_end, res.query_begin, res.query_end = score, rb, re_, qb, qe
        res.score2 = res.ref_end2 = None
        res.cigar_string = None
        if report_cigar:
            tail = query_lens[k] - qe - 1
            res.cigar_string = ('%dS' % qb if qb > 0 else '') + ''.join('%d%s' % (c, o) for o, c in ops) + ('%dS' % tail if tail else '')
        if banded:
            res.band_exact = bool(halves[2 * k].band_exact and halves[2 * k + 1].band_exact)
        out.append(res)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the pair family against windows of the resident genome (hip.Genome): K1g, K1gb, spliced, extension from anchors
# ---------------------------------------------------------------------------------------------------------------------------
GATHER_REVERSE, GATHER_COMPLEMENT = 1, 2      # window flags of hip.EndsPlan(windows=...) / hip.BandPlan(windows=...); 3: the minus strand


def _window_spans(who, genome, windows):
    """[(contig, start, end)] -> (genome-wide offsets int64, lengths int64); ValueError names the first window that is not
    0 <= start <= end <= length of a resident contig"""
    off = np.zeros(len(windows), dtype=np.int64); ln = np.zeros(len(windows), dtype=np.int64)
    for k, w in enumerate(windows):
        ctg, a, b = w[0], int(w[1]), int(w[2])
        if ctg not in genome.offset:
            raise ValueError('%s: window %d %r: contig %r is not resident' % (who, k, tuple(w), ctg))
        if not 0 <= a <= b <= genome.length[ctg]:
            raise ValueError('%s: window %d %r lies outside contig %r of %d bases (0 <= start <= end <= length)' % (who, k, tuple(w), ctg, genome.length[ctg]))
        off[k] = genome.offset[ctg] + a; ln[k] = b - a
    return off, ln


def _window_coords(res, contig, start, length, minus):
    """contig, minus, genome_begin, genome_end on a result whose ref_begin / ref_end are relative to the window [start, start + length)
    as it was read: forwards, or as the minus strand (letter t = base start + length - 1 - t).  0-based, inclusive, forward-strand
    contig coordinates; a span without a letter keeps genome_end == genome_begin - 1"""
    res.contig, res.minus = contig, bool(minus)
    if minus:
        res.genome_begin, res.genome_end = start + length - 1 - res.ref_end, start + length - 1 - res.ref_begin
    else:
        res.genome_begin, res.genome_end = start + res.ref_begin, start + res.ref_end
    return res


def _exons_of(cigar_string, genome_begin):
    """the exons of a spliced CIGAR whose first reference letter is contig position genome_begin (forward strand): [(start, end)],
    inclusive, ascending, split at N; M and D lie inside an exon, I and S take no reference letter"""
    exons, pos, first, num = [], genome_begin, genome_begin, ''
    for ch in cigar_string or '':
        if ch.isdigit():
            num += ch
            continue
        k, num = int(num), ''
        if ch in 'MD=X':
            pos += k
        elif ch == 'N':
            if pos > first:
                exons.append((first, pos - 1))
            pos += k
            first = pos
    if pos > first:
        exons.append((first, pos - 1))
    return exons


def _genome_context(who, genome, context):
    if context is not None and context is not genome.ctx:
        raise ValueError('%s: the genome lives on another context' % who)
    return genome.ctx


def align_windows_ends(genome, windows, minus, query_seqs, mode='global', match=2, mismatch=2, gap_open=3, gap_extend=1, report_cigar=False,
                       context=None, gap_open2=None, gap_extend2=None, traceback='stored'):
    """``align_pairs_ends`` with reference k = window (contig, start, end) of a genome resident on the GPU (hip.Genome), read as the
    minus strand where minus[k]: element k equals ``align_pairs_ends`` on the window's string, upper-cased and, where minus[k],
    reverse-complemented -- the same scores, ties and CIGARs, with no string sliced, reversed, encoded or uploaded: the device
    gathers the windows into the plan's reference buffer (csrc/genome_gather.h).  Unlike ``align_windows``, which keeps the
    reference's revcomp() quirk, lower-case bases ARE complemented on the minus strand: a soft-masked exon aligns.  DNA match /
    mismatch only (no `matrix`, no `alphabet`); every other keyword is ``align_pairs_ends``'s.

    ref_begin and ref_end are relative to the window as read.  Each result also carries ``contig``, ``minus``, ``genome_begin`` and
    ``genome_end``: 0-based, inclusive, forward-strand contig coordinates (on a minus window genome_begin = start + L - 1 -
    ref_end); an empty span keeps genome_end == genome_begin - 1.  A window that is not 0 <= start <= end <= genome.length[contig],
    or whose contig is not resident, is a ValueError that names it."""
    who = 'align_windows_ends'
    two = {} if hip.gap2_of(who, gap_open2, gap_extend2) is None else dict(gap_open2=gap_open2, gap_extend2=gap_extend2)
    if traceback not in hip.ENDS_TRACEBACKS:
        raise ValueError("%s: traceback must be 'stored' or 'recompute', got %r" % (who, traceback))
    if mode not in hip.ENDS_MODES:
        raise ValueError("%s: mode must be 'global', 'semiglobal', 'overlap', 'prefix' or 'extend', got %r" % (who, mode))
    n = len(windows)
    if len(query_seqs) != n or len(minus) != n:
        raise ValueError('%s: %d windows vs %d strands vs %d queries' % (who, n, len(minus), len(query_seqs)))
    off, ln = _window_spans(who, genome, windows)
    ctx = _genome_context(who, genome, context)
    if not n:
        return []
    mat, (qd, qo), _ = _pairs_inputs(who, [], query_seqs, match, mismatch, None, None)
    flags = np.where(np.asarray(minus, dtype=bool), GATHER_REVERSE | GATHER_COMPLEMENT, 0).astype(np.uint8)
    walk = bool(report_cigar) or mode in ('semiglobal', 'overlap')
    rows, cig = ctx.ends_batch(qd, qo, None, None, mat, gap_open, gap_extend, mode=mode, want_cigar=walk, traceback=traceback, windows=(genome, off, ln, flags), **two)
    out = _pairs_results(rows, cig, qo, walk, report_cigar)
    for k, res in enumerate(out):
        _window_coords(res, windows[k][0], int(windows[k][1]), int(ln[k]), minus[k])
    return out


def align_windows_band(genome, windows, minus, query_seqs, band, mode='global', diagonals=None, match=2, mismatch=2, gap_open=3, gap_extend=1,
                       report_cigar=False, context=None, gap_open2=None, gap_extend2=None):
    """``align_pairs_band`` with reference k = window (contig, start, end) of a resident genome, read as the minus strand where
    minus[k] (diagonals are those of the window as read): the results of ``align_pairs_band`` on the windows' strings, ``band`` and
    ``band_exact`` included, with the genome coordinates and the lower-case rule of ``align_windows_ends``."""
    who = 'align_windows_band'
    two = {} if hip.gap2_of(who, gap_open2, gap_extend2) is None else dict(gap_open2=gap_open2, gap_extend2=gap_extend2)
    if mode not in ('global', 'semiglobal', 'prefix', 'extend'):
        raise ValueError("%s: mode must be 'global', 'semiglobal', 'prefix' or 'extend'%s, got %r"
                         % (who, " ('overlap' with a band is not built)" if mode == 'overlap' else '', mode))
    n = len(windows)
    if len(query_seqs) != n or len(minus) != n:
        raise ValueError('%s: %d windows vs %d strands vs %d queries' % (who, n, len(minus), len(query_seqs)))
    if diagonals is not None and len(diagonals) != n:
        raise ValueError('%s: %d diagonals vs %d pairs' % (who, len(diagonals), n))
    if int(band) != band or band < 0:
        raise ValueError('%s: band is a half-width in diagonals, an integer >= 0, got %r' % (who, band))
    off, ln = _window_spans(who, genome, windows)
    ctx = _genome_context(who, genome, context)
    if not n:
        return []
    mat, (qd, qo), _ = _pairs_inputs(who, [], query_seqs, match, mismatch, None, None)
    flags = np.where(np.asarray(minus, dtype=bool), GATHER_REVERSE | GATHER_COMPLEMENT, 0).astype(np.uint8)
    walk = bool(report_cigar) or mode == 'semiglobal'
    rows, cig = ctx.band_batch(qd, qo, None, None, mat, gap_open, gap_extend, int(band), mode=mode, diagonals=diagonals, want_cigar=walk,
                               windows=(genome, off, ln, flags), **two)
    out = _pairs_results(rows, cig, qo, walk, report_cigar)
    for k, (r, res) in enumerate(zip(rows, out)):
        res.band = (int(r['band_lo']), int(r['band_hi']))
        res.band_exact = bool(r['exact'])
        _window_coords(res, windows[k][0], int(windows[k][1]), int(ln[k]), minus[k])
    return out


def align_windows_spliced(genome, windows, query_seqs, mode='semiglobal', strand='+', match=2, mismatch=2, gap_open=3, gap_extend=1, intron_open=12,
                          noncanonical=6, donor_costs=None, acceptor_costs=None, report_cigar=False, context=None, traceback='stored'):
    """``align_pairs_spliced`` with reference k = window (contig, start, end) of a resident genome.  The window is always read on the
    forward strand; `strand` is the transcript's, exactly as in ``align_pairs_spliced`` ('+', '-', one per pair, or 'both': pairs k
    and n + k of one plan, each window gathered twice, the higher score kept, ties to '+').  The results are those of
    ``align_pairs_spliced`` on the windows' upper-cased strings, ``strand`` included, with ``contig``, ``minus`` (False),
    ``genome_begin`` and ``genome_end`` as ``align_windows_ends`` gives them; with report_cigar also ``exons``: the forward-strand
    contig intervals [(start, end), ...], inclusive and ascending, that the CIGAR's N ops split the alignment into -- what
    ``align.get_exons`` would be asked for next."""
    who = 'align_windows_spliced'
    if traceback not in hip.ENDS_TRACEBACKS:
        raise ValueError("%s: traceback must be 'stored' or 'recompute', got %r" % (who, traceback))
    if mode not in hip.ENDS_MODES:
        raise ValueError("%s: mode must be 'global', 'semiglobal', 'overlap', 'prefix' or 'extend', got %r" % (who, mode))
    n = len(windows)
    if len(query_seqs) != n:
        raise ValueError('%s: %d windows vs %d queries' % (who, n, len(query_seqs)))
    if min(int(match), int(mismatch), int(gap_open), int(gap_extend)) < 0:
        raise ValueError('%s: match, mismatch and the gap costs must not be negative' % who)
    splice = hip.splice_of(who, intron_open, noncanonical, donor_costs, acceptor_costs)
    both = isinstance(strand, str) and strand == 'both'
    st = np.concatenate([np.ones(n, dtype=np.int8), -np.ones(n, dtype=np.int8)]) if both else _strands(strand, n)
    off, ln = _window_spans(who, genome, windows)
    ctx = _genome_context(who, genome, context)
    if not n:
        return []
    queries = list(query_seqs) * 2 if both else query_seqs
    if both:
        off, ln = np.concatenate([off, off]), np.concatenate([ln, ln])
    mat, (qd, qo), _ = _pairs_inputs(who, [], queries, match, mismatch, None, None)
    walk = bool(report_cigar) or mode in ('semiglobal', 'overlap')
    rows, cig = ctx.ends_batch(qd, qo, None, None, mat, gap_open, gap_extend, mode=mode, want_cigar=walk, splice=splice, strand=st, traceback=traceback,
                               windows=(genome, off, ln, np.zeros(len(off), dtype=np.uint8)))
    out = _pairs_results(rows, cig, qo, walk, report_cigar)
    for k, (res, s) in enumerate(zip(out, st)):
        res.strand = '+' if s > 0 else '-'
        w = windows[k % n]
        _window_coords(res, w[0], int(w[1]), int(ln[k]), False)
        if report_cigar:
            res.exons = _exons_of(res.cigar_string, res.genome_begin)
    if both:
        out = [out[k] if out[k].score >= out[n + k].score else out[n + k] for k in range(n)]
    return out


def _anchor_flanks(contig_len, pos, query_pos, query_len, slack, minus):
    """(left_flank, right_flank, start): the reference letters in front of and behind the anchor as the query reads them, and the
    first base of the contig interval [start, start + left_flank + right_flank) they come from.  A side holds the query letters on
    that side plus `slack`, or what the contig has.  On the plus strand the query's left is towards base 0; on the minus strand the
    query reads the reverse complement, so its left is towards the contig's end"""
    lo_room, hi_room = pos, contig_len - pos
    left = min(hi_room if minus else lo_room, query_pos + slack)
    right = min(lo_room if minus else hi_room, query_len - query_pos + slack)
    return left, right, pos - (right if minus else left)


def extend_anchors_genome(genome, anchors, minus, query_seqs, band=None, slack=None, match=2, mismatch=2, gap_open=3, gap_extend=1, report_cigar=False,
                          context=None, gap_open2=None, gap_extend2=None, traceback='stored'):
    """``extend_anchors`` along a resident genome: anchors[k] = (contig, pos, query_pos) is a point between letters, `pos` on the
    forward strand of the contig (between bases pos - 1 and pos), query_pos in the query; where minus[k] the query reads the minus
    strand.  On each side of the anchor, as the query reads it, the reference flank is min(letters to the contig's edge, query
    letters on that side + slack); slack defaults to 64, with a band to `band`.  The 2 n flanks are 2 n windows of one plan, none of
    them a string: the left half of a plus-strand anchor is gathered reversed (flags 1), its right half as it stands; for a
    minus-strand anchor the right half is the bases below pos reversed and complemented (flags 3) and the left half the bases from
    pos on complemented (flags 2).  Only the query's left part is reversed on the host.  There is no seed_len: a seed's letters are
    the first columns of the right half.

    Definition: with (left, right) the two flanks, the result equals ``extend_anchors`` on the strand-resolved string of the contig
    interval [pos - left, pos + right) -- on the minus strand the reverse complement of [pos - right, pos + left) -- upper-cased,
    with anchor (left, query_pos): ref_begin and ref_end are relative to that string, ``band_exact`` as there.  ``contig``,
    ``minus``, ``genome_begin`` and ``genome_end`` are those of ``align_windows_ends`` for that interval."""
    who = 'extend_anchors_genome'
    two = {} if hip.gap2_of(who, gap_open2, gap_extend2) is None else dict(gap_open2=gap_open2, gap_extend2=gap_extend2)
    if traceback not in hip.ENDS_TRACEBACKS:
        raise ValueError("%s: traceback must be 'stored' or 'recompute', got %r" % (who, traceback))
    if traceback != 'stored' and band is not None:
        raise ValueError("%s: traceback=%r goes with band=None: K1gb has the stored route alone" % (who, traceback))
    n = len(anchors)
    if len(query_seqs) != n or len(minus) != n:
        raise ValueError('%s: %d anchors vs %d strands vs %d queries' % (who, n, len(minus), len(query_seqs)))
    if band is not None and (int(band) != band or band < 0):
        raise ValueError('%s: band is a half-width in diagonals, an integer >= 0, got %r' % (who, band))
    if slack is None:
        slack = 64 if band is None else int(band)
    if int(slack) != slack or slack < 0:
        raise ValueError('%s: slack is a number of letters >= 0, got %r' % (who, slack))
    windows2, flags2, queries2, spans, local = [], [], [], [], []
    for k in range(n):
        ctg, pos, qp = anchors[k][0], int(anchors[k][1]), int(anchors[k][2])
        q = query_seqs[k]
        if ctg not in genome.offset:
            raise ValueError('%s: anchor %d %r: contig %r is not resident' % (who, k, tuple(anchors[k]), ctg))
        if not (0 <= pos <= genome.length[ctg] and 0 <= qp <= len(q)):
            raise ValueError('%s: anchor %d %r lies outside contig %r of %d bases or the query of %d letters'
                             % (who, k, tuple(anchors[k]), ctg, genome.length[ctg], len(q)))
        left, right, start = _anchor_flanks(genome.length[ctg], pos, qp, len(q), int(slack), bool(minus[k]))
        if minus[k]:
            windows2 += [(ctg, pos, pos + left), (ctg, pos - right, pos)]
            flags2 += [GATHER_COMPLEMENT, GATHER_REVERSE | GATHER_COMPLEMENT]
        else:
            windows2 += [(ctg, pos - left, pos), (ctg, pos, pos + right)]
            flags2 += [GATHER_REVERSE, 0]
        queries2 += [q[:qp][::-1], q[qp:]]
        spans.append((ctg, start, left + right)); local.append((left, qp))
    off, ln = _window_spans(who, genome, windows2)
    ctx = _genome_context(who, genome, context)
    if not n:
        return []
    mat, (qd, qo), _ = _pairs_inputs(who, [], queries2, match, mismatch, None, None)
    wins = (genome, off, ln, np.array(flags2, dtype=np.uint8))
    if band is None:
        rows, cig = ctx.ends_batch(qd, qo, None, None, mat, gap_open, gap_extend, mode='extend', want_cigar=bool(report_cigar), traceback=traceback, windows=wins, **two)
    else:
        rows, cig = ctx.band_batch(qd, qo, None, None, mat, gap_open, gap_extend, int(band), mode='extend', want_cigar=bool(report_cigar), windows=wins, **two)
    halves = _pairs_results(rows, cig, qo, bool(report_cigar), report_cigar)
    if band is not None:
        for r, res in zip(rows, halves):
            res.band_exact = bool(r['exact'])
    out = _stitch_halves(halves, local, [len(q) for q in query_seqs], 0, [0] * n, report_cigar, band is not None)
    for k, res in enumerate(out):
        _window_coords(res, spans[k][0], spans[k][1], spans[k][2], minus[k])
    return out
