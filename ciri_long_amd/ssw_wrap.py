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
    of the reference) or 'overlap' (end gaps free on both sequences) -- under the same affine scores, DNA or matrix (K1g);
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


def align_pairs_ends(ref_seqs, query_seqs, mode='global', match=2, mismatch=2, gap_open=3, gap_extend=1, report_cigar=False, matrix=None,
                     alphabet=None, context=None):
    """n independent (reference, query) alignments anchored at the ends, in one GPU call -> one PyAlignRes per pair.

    mode 'global': both sequences end to end.  'semiglobal': the whole query in any stretch of the reference (a probe, an exon, a
    junction placed inside a read).  'overlap': end gaps free on both sequences at both ends (dovetails, containment).  Scores are
    those of ``align_pairs`` -- match / mismatch, or `matrix` (n x n, row = reference letter) over `alphabet` as in
    ``align_pairs_matrix`` -- with a gap of k letters costing gap_open + (k - 1) gap_extend, gap_open >= gap_extend.

    ``score`` may be negative.  Coordinates are 0-based and inclusive; a span that consumed no letter has end == begin - 1.  Ties: the
    semiglobal end is the smallest reference column with the best score; the overlap end is sought in the last row first (smallest
    column), then in the last column (smallest row); the walk back prefers the diagonal, then a reference letter against nothing
    (D), then a query letter against nothing (I), and leaves a gap as soon as it can.  ``score2`` and ``ref_end2`` are None.
    ``cigar_string`` (report_cigar) uses M / I / D, with soft clips for the query letters outside query_begin..query_end as
    ``align_pairs`` writes them.  Parity with other libraries' tie rules is not pinned."""
    if mode not in hip.ENDS_MODES:
        raise ValueError("align_pairs_ends: mode must be 'global', 'semiglobal' or 'overlap', got %r" % (mode,))
    if len(ref_seqs) != len(query_seqs):
        raise ValueError('align_pairs_ends: %d references vs %d queries' % (len(ref_seqs), len(query_seqs)))
    mat, (qd, qo), (rd, ro) = _pairs_inputs('align_pairs_ends', ref_seqs, query_seqs, match, mismatch, matrix, alphabet)
    if not ref_seqs:
        return []
    ctx = context or hip.default_context()
    walk = bool(report_cigar) or mode != 'global'          # the begins come from the walk, unless the mode fixes them
    rows, cig = ctx.ends_batch(qd, qo, rd, ro, mat, gap_open, gap_extend, mode=mode, want_cigar=walk)
    return _pairs_results(rows, cig, qo, walk, report_cigar)


def align_pairs_band(ref_seqs, query_seqs, band, mode='global', diagonals=None, match=2, mismatch=2, gap_open=3, gap_extend=1, report_cigar=False,
                     matrix=None, alphabet=None, context=None):
    """``align_pairs_ends`` over a band of diagonals, in one GPU call -> one PyAlignRes per pair.

    With i query and j reference letters consumed, only cells with lo <= j - i <= hi exist: lo = min(0, n - m) - band and hi =
    max(0, n - m) + band (the corner diagonals of the m x n pair widened by `band`), or diagonals[k] - band and diagonals[k] + band
    where a placement is known (a seed, a minimizer hit, an ``edlib.search`` location: the diagonal is reference position minus
    query position); both clipped to [-m, n], at most 512 diagonals.  mode is 'global' or 'semiglobal'; scores, coordinates, tie
    rules and the CIGAR are those of ``align_pairs_ends``, and every result is the best alignment that stays inside the band.  Each
    result also carries ``band`` = (lo, hi) as clipped, and ``band_exact``: True where it is proved that ``align_pairs_ends`` returns
    the same result and CIGAR (False: not proved; they may still be equal).  The cost is m x (hi - lo + 1) cells, not m x n, and
    CIGARs need half a byte per cell of the band.  A band that holds no alignment, 'overlap', and a band above 512 diagonals raise
    hip.ClhError."""
    if mode not in ('global', 'semiglobal'):
        raise ValueError("align_pairs_band: mode must be 'global' or 'semiglobal'%s, got %r"
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
    walk = bool(report_cigar) or mode != 'global'          # the begins come from the walk, unless the mode fixes them
    rows, cig = ctx.band_batch(qd, qo, rd, ro, mat, gap_open, gap_extend, int(band), mode=mode, diagonals=diagonals, want_cigar=walk)
    out = _pairs_results(rows, cig, qo, walk, report_cigar)
    for r, res in zip(rows, out):
        res.band = (int(r['band_lo']), int(r['band_hi']))
        res.band_exact = bool(r['exact'])
    return out
