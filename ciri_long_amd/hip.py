"""ctypes binding of libclh.so's batched C ABI (include/ciri_long_hip.h).

The shared object is built in-tree by csrc/Makefile (``python -c 'import __graft_entry__ as g; g.build()'``) and must
sit next to this file, as the reference's libssw.so sits next to its wrapper (ssw_wrap.py:17).  Nothing here falls
back to the CPU: a missing library or GPU raises ``HipUnavailable``.
"""
import ctypes as C
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get('CLH_LIB') or os.path.join(_HERE, 'libclh.so')     # CLH_LIB: another build of the same ABI (kernel experiments)


class HipUnavailable(RuntimeError):
    pass


class ClhError(RuntimeError):
    pass


class AlignRow(C.Structure):
    _fields_ = [('score1', C.c_uint16), ('score2', C.c_uint16), ('ref_begin1', C.c_int32), ('ref_end1', C.c_int32),
                ('read_begin1', C.c_int32), ('read_end1', C.c_int32), ('ref_end2', C.c_int32),
                ('cigar_off', C.c_int32), ('cigar_len', C.c_int32), ('status', C.c_int32)]


ALIGN_DTYPE = np.dtype([('score1', '<u2'), ('score2', '<u2'), ('ref_begin1', '<i4'), ('ref_end1', '<i4'),
                        ('read_begin1', '<i4'), ('read_end1', '<i4'), ('ref_end2', '<i4'), ('cigar_off', '<i4'),
                        ('cigar_len', '<i4'), ('status', '<i4')])
assert ALIGN_DTYPE.itemsize == C.sizeof(AlignRow)

ST_WORD, ST_NULL, ST_TRACE_ERR, ST_NO_CIGAR, ST_CIGAR_TRUNC = 1, 2, 4, 8, 16

CCS_SEG_CAP = 65
CCS_DTYPE = np.dtype([('nseg', '<i4'), ('ccs_len', '<i4'), ('period', '<i4'), ('status', '<i4')])


class SswOpts(C.Structure):
    _fields_ = [('mat', C.c_void_p), ('n_mat', C.c_int32), ('gap_open', C.c_uint8), ('gap_extend', C.c_uint8),
                ('flag', C.c_uint8), ('score_size', C.c_int8), ('filters', C.c_uint16), ('filterd', C.c_int32),
                ('want_score2', C.c_int32), ('want_cigar', C.c_int32)]


class EditAlignOpts(C.Structure):
    _fields_ = [('mode', C.c_int32), ('task', C.c_int32), ('k', C.c_int32), ('n_eq', C.c_int32), ('eq', C.c_void_p),
                ('workspace_bytes', C.c_int64)]


class EditSearchOpts(C.Structure):
    _fields_ = [('k', C.c_int32), ('n_eq', C.c_int32), ('eq', C.c_void_p)]


class EndsOpts(C.Structure):
    _fields_ = [('mode', C.c_int32), ('mat', C.c_void_p), ('n_mat', C.c_int32), ('gap_open', C.c_int32), ('gap_extend', C.c_int32),
                ('want_cigar', C.c_int32), ('workspace_bytes', C.c_int64)]


class Gap2(C.Structure):
    _fields_ = [('gap_open2', C.c_int32), ('gap_extend2', C.c_int32)]


def gap2_of(who, gap_open2, gap_extend2):
    """the second piece of two-piece gap costs as libclh takes it -> Gap2, or None for one piece; the two come together"""
    if (gap_open2 is None) != (gap_extend2 is None):
        raise ValueError('%s: gap_open2 and gap_extend2 come together' % who)
    return None if gap_open2 is None else Gap2(int(gap_open2), int(gap_extend2))


class Splice(C.Structure):
    _fields_ = [('intron_open', C.c_int32), ('donor', C.c_int32 * 16), ('acceptor', C.c_int32 * 16), ('other', C.c_int32)]


def splice_of(who, intron_open, noncanonical, donor_costs=None, acceptor_costs=None):
    """the intron costs as libclh takes them (clh_splice): GT as donor and AG as acceptor cost 0, every other dinucleotide, and one
    that holds an N or runs off the reference, cost `noncanonical`; the dicts override single dinucleotides as read on the transcript
    strand, e.g. {'GC': 2}"""
    sp = Splice()
    if int(intron_open) < 0 or int(noncanonical) < 0:
        raise ValueError('%s: intron_open and noncanonical must not be negative' % who)
    sp.intron_open, sp.other = int(intron_open), int(noncanonical)
    for table, free, over, name in ((sp.donor, 'GT', donor_costs, 'donor_costs'), (sp.acceptor, 'AG', acceptor_costs, 'acceptor_costs')):
        for k in range(16):
            table[k] = int(noncanonical)
        table[4 * 'ACGT'.index(free[0]) + 'ACGT'.index(free[1])] = 0
        for key, v in (over or {}).items():
            key = str(key).upper()
            if len(key) != 2 or key[0] not in 'ACGT' or key[1] not in 'ACGT':
                raise ValueError('%s: %s names dinucleotides over ACGT, got %r' % (who, name, key))
            if int(v) < 0:
                raise ValueError('%s: %s[%r] must not be negative' % (who, name, key))
            table[4 * 'ACGT'.index(key[0]) + 'ACGT'.index(key[1])] = int(v)
    return sp


ENDS_DTYPE = np.dtype([('score', '<i4'), ('ref_begin', '<i4'), ('ref_end', '<i4'), ('query_begin', '<i4'), ('query_end', '<i4'),
                       ('cigar_len', '<i4'), ('cigar_off', '<i8')])
ENDS_MODES = {'global': 0, 'semiglobal': 1, 'overlap': 2, 'prefix': 3, 'extend': 4}
ENDS_TRACEBACKS = {'stored': 1, 'recompute': 2}      # clh_ends_opts.want_cigar: CLH_ENDS_CIGAR_STORED, CLH_ENDS_CIGAR_RECOMPUTE


class BandOpts(C.Structure):
    _fields_ = [('mode', C.c_int32), ('mat', C.c_void_p), ('n_mat', C.c_int32), ('gap_open', C.c_int32), ('gap_extend', C.c_int32),
                ('want_cigar', C.c_int32), ('workspace_bytes', C.c_int64), ('band', C.c_int32), ('reserved', C.c_int32)]


class ChainOpts(C.Structure):
    _fields_ = [('lookback', C.c_int32), ('max_chains', C.c_int32), ('max_attempts', C.c_int32), ('min_score', C.c_int32), ('min_anchors', C.c_int32),
                ('reserved', C.c_int32), ('max_gap', C.c_int64), ('max_skew', C.c_int64), ('workspace_bytes', C.c_int64)]


class LinkOpts(C.Structure):
    _fields_ = [('max_query_gap', C.c_int64), ('max_overlap', C.c_int64), ('max_skew', C.c_int64), ('max_intron', C.c_int64), ('max_circle', C.c_int64),
                ('intron_cost', C.c_int64), ('backsplice_cost', C.c_int64)]


class JunctionOpts(C.Structure):
    _fields_ = [('match', C.c_int32), ('mismatch', C.c_int32), ('gap_open', C.c_int32), ('gap_extend', C.c_int32), ('slack', C.c_int32), ('max_span', C.c_int32)]


BAND_DTYPE = np.dtype([('score', '<i4'), ('ref_begin', '<i4'), ('ref_end', '<i4'), ('query_begin', '<i4'), ('query_end', '<i4'),
                       ('cigar_len', '<i4'), ('cigar_off', '<i8'), ('band_lo', '<i4'), ('band_hi', '<i4'), ('exact', '<i4'), ('reserved', '<i4')])
EDIT_SEARCH_DTYPE = np.dtype([('distance', '<i4'), ('start', '<i4'), ('end', '<i4'), ('last_end', '<i4'), ('nlocs', '<i4')])
EDIT_ALIGN_DTYPE = np.dtype([('distance', '<i4'), ('nlocs', '<i4'), ('loc_off', '<i8'), ('cigar_off', '<i8'), ('cigar_len', '<i4'),
                             ('status', '<i4'), ('alphabet_len', '<i4'), ('reserved', '<i4')])
EA_MODES = {'NW': 0, 'SHW': 1, 'HW': 2}
EA_TASKS = {'distance': 0, 'locations': 1, 'path': 2}
EA_ST_ABOVE_K = 1


_lib = None
_gpu_used = False         # set when this process creates its first device context (clh_create: the first call that initialises the HIP runtime);
                          # loading libclh.so and its host-only entry points (fastx_index, fastx_count, encode) do not


def lib():
    """Load libclh.so (once).  Raises HipUnavailable if it has not been built."""
    global _lib
    if _lib is None:
        if os.environ.get('CIRI_LONG_MAPPER_WORKER') == '1':
            raise HipUnavailable('a mapper worker process must not touch the GPU (ciri_long_amd/mapper_pool.py)')
        if not os.path.exists(SO_PATH):
            raise HipUnavailable('%s not found: build it with `make -C %s/csrc` (needs hipcc); there is no CPU fallback'
                                 % (SO_PATH, _HERE))
        L = C.CDLL(SO_PATH)
        L.clh_last_error.restype = C.c_char_p
        L.clh_version.restype = C.c_char_p
        L.clh_create.restype = C.c_void_p
        L.clh_create.argtypes = [C.c_int]
        L.clh_destroy.argtypes = [C.c_void_p]
        L.clh_ssw_plan.restype = C.c_void_p
        L.clh_ssw_plan.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(SswOpts)]
        L.clh_plan_destroy.argtypes = [C.c_void_p]
        L.clh_ssw_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.clh_ssw_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
        L.clh_ssw_results_dev.restype = C.c_void_p
        L.clh_ssw_results_dev.argtypes = [C.c_void_p]
        L.clh_ssw_batch.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.POINTER(SswOpts), C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
        L.clh_encode_dna.argtypes = [C.c_char_p, C.c_int64, C.c_void_p]
        L.clh_ccs_plan_create.restype = C.c_void_p
        L.clh_ccs_plan_create.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        L.clh_ccs_plan_destroy.argtypes = [C.c_void_p]
        L.clh_ccs_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.clh_ccs_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.clh_ccs_batch.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.clh_ccs_plan_timing.argtypes = [C.c_void_p, C.c_void_p]
        L.clh_ccs_file.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_char_p, C.c_char_p, C.c_int32, C.c_void_p]
        L.clh_ccs_file.restype = C.c_int
        L.clh_ccs_file_range.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_char_p, C.c_char_p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p]
        L.clh_ccs_file_range.restype = C.c_int
        L.clh_fastx_count.argtypes = [C.c_char_p, C.c_int, C.c_void_p]
        L.clh_genome_create.restype = C.c_void_p
        L.clh_genome_create.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
        L.clh_genome_destroy.restype = None
        L.clh_genome_destroy.argtypes = [C.c_void_p]
        L.clh_genome_codes.restype = C.c_void_p
        L.clh_genome_codes.argtypes = [C.c_void_p]
        L.clh_genome_length.restype = C.c_int64
        L.clh_genome_length.argtypes = [C.c_void_p]
        L.clh_genome_count_n.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.clh_genome_set_splice_sites.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.clh_splice_signal_batch.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
        L.clh_ssw_plan_windows.restype = C.c_void_p
        L.clh_ssw_plan_windows.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.clh_ssw_windows_batch.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        L.clh_edit_plan_create.restype = C.c_void_p
        L.clh_edit_plan_create.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.clh_edit_plan_destroy.restype = None
        L.clh_edit_plan_destroy.argtypes = [C.c_void_p]
        L.clh_edit_plan_run.argtypes = [C.c_void_p, C.c_void_p]
        L.clh_edit_plan_fetch.argtypes = [C.c_void_p, C.c_void_p]
        L.clh_edit_plan_timing.argtypes = [C.c_void_p, C.c_void_p]
        L.clh_edit_distance_batch.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.clh_edit_distance_batch.restype = C.c_int
        L.clh_edit_matrix_plan_create.restype = C.c_void_p
        L.clh_edit_matrix_plan_create.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]
        L.clh_edit_matrix_plan_destroy.restype = None
        L.clh_edit_matrix_plan_destroy.argtypes = [C.c_void_p]
        L.clh_edit_matrix_plan_run.argtypes = [C.c_void_p, C.c_void_p]
        L.clh_edit_matrix_plan_sizes.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.clh_edit_matrix_plan_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64]
        L.clh_edit_matrix_plan_timing.argtypes = [C.c_void_p, C.c_void_p]
        L.clh_edit_matrix_batch.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64,
                                            C.c_void_p, C.c_void_p, C.c_int64]
        L.clh_edit_align_plan_create.restype = C.c_void_p
        L.clh_edit_align_plan_create.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(EditAlignOpts)]
        L.clh_edit_align_plan_destroy.restype = None
        L.clh_edit_align_plan_destroy.argtypes = [C.c_void_p]
        L.clh_edit_align_plan_run.argtypes = [C.c_void_p, C.c_void_p]
        L.clh_edit_align_plan_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.c_void_p, C.c_int64,
                                                C.POINTER(C.c_int64)]
        L.clh_edit_align_plan_timing.argtypes = [C.c_void_p, C.c_void_p]
        L.clh_edit_align_plan_caps.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.clh_edit_align_batch.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(EditAlignOpts),
                                           C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
        L.clh_edit_search_plan_create.restype = C.c_void_p
        L.clh_edit_search_plan_create.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                                  C.POINTER(EditSearchOpts)]
        L.clh_edit_search_plan_destroy.restype = None
        L.clh_edit_search_plan_destroy.argtypes = [C.c_void_p]
        L.clh_edit_search_plan_run.argtypes = [C.c_void_p, C.c_void_p]
        L.clh_edit_search_plan_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        L.clh_edit_search_plan_timing.argtypes = [C.c_void_p, C.c_void_p]
        L.clh_edit_search_plan_info.argtypes = [C.c_void_p, C.c_void_p]
        L.clh_edit_search_batch.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                            C.POINTER(EditSearchOpts), C.c_void_p, C.c_int64]
        L.clh_ends_plan_create.restype = C.c_void_p
        L.clh_ends_plan_create.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(EndsOpts)]
        L.clh_ends_plan_destroy.restype = None
        L.clh_ends_plan_destroy.argtypes = [C.c_void_p]
        L.clh_ends_plan_run.argtypes = [C.c_void_p, C.c_void_p]
        L.clh_ends_plan_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
        L.clh_ends_plan_timing.argtypes = [C.c_void_p, C.c_void_p]
        L.clh_ends_plan_info.argtypes = [C.c_void_p, C.c_void_p]
        L.clh_ends_batch.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(EndsOpts), C.c_void_p,
                                     C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
        if hasattr(L, 'clh_ends_plan_create_gap2'):      # absent from a CLH_LIB build older than the two-piece gap costs: using them there raises
            L.clh_ends_plan_create_gap2.restype = C.c_void_p
            L.clh_ends_plan_create_gap2.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(EndsOpts),
                                                    C.POINTER(Gap2)]
            L.clh_ends_batch_gap2.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(EndsOpts), C.POINTER(Gap2),
                                              C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
            L.clh_band_batch_gap2.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(BandOpts),
                                              C.POINTER(Gap2), C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
            L.clh_band_plan_create_gap2.restype = C.c_void_p
            L.clh_band_plan_create_gap2.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(BandOpts),
                                                    C.POINTER(Gap2)]
        if hasattr(L, 'clh_ends_plan_create_spliced'):   # absent from a CLH_LIB build older than spliced alignment: using it there raises
            L.clh_ends_plan_create_spliced.restype = C.c_void_p
            L.clh_ends_plan_create_spliced.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(EndsOpts),
                                                       C.POINTER(Splice), C.c_void_p]
            L.clh_ends_batch_spliced.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(EndsOpts), C.POINTER(Splice),
                                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
        if hasattr(L, 'clh_ends_plan_create_windows'):   # absent from a CLH_LIB build older than pair plans on genome windows: using them there raises
            L.clh_ends_plan_create_windows.restype = C.c_void_p
            L.clh_ends_plan_create_windows.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(EndsOpts),
                                                       C.POINTER(Gap2), C.POINTER(Splice), C.c_void_p]
            L.clh_ends_plan_gather_timing.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int64)]
            L.clh_band_plan_gather_timing.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int64)]
            L.clh_band_plan_create_windows.restype = C.c_void_p
            L.clh_band_plan_create_windows.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                       C.POINTER(BandOpts), C.POINTER(Gap2)]
        if hasattr(L, 'clh_seed_index_create'):          # absent from a CLH_LIB build older than the minimizer index (K7): SeedIndex raises there
            L.clh_seed_index_create.restype = C.c_void_p
            L.clh_seed_index_create.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32]
            L.clh_seed_index_destroy.restype = None
            L.clh_seed_index_destroy.argtypes = [C.c_void_p]
            L.clh_seed_index_info.argtypes = [C.c_void_p, C.c_void_p]
            L.clh_seed_index_timing.argtypes = [C.c_void_p, C.c_void_p]
            L.clh_seed_index_dump.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
            L.clh_seed_minimizers.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
            L.clh_seed_minimizers_fetch.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
            L.clh_seed_batch.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
            L.clh_seed_batch_fetch.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
            L.clh_seed_chain_batch.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(ChainOpts), C.c_void_p, C.c_void_p]
        if hasattr(L, 'clh_seed_link_batch'):            # absent from a CLH_LIB build older than the links between chains: links() raises there
            L.clh_seed_link_batch.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(ChainOpts), C.POINTER(LinkOpts), C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p]
            L.clh_seed_link_rows.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(LinkOpts), C.c_void_p, C.c_void_p]
        if hasattr(L, 'clh_seed_junction_batch'):        # absent from a CLH_LIB build older than the junction refinement: junctions() raises there
            L.clh_seed_junction_batch.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(JunctionOpts), C.POINTER(Splice),
                                                  C.c_void_p, C.POINTER(C.c_float)]
            L.clh_seed_junction_info.argtypes = [C.c_void_p]
            L.clh_genome_letters.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        if hasattr(L, 'clh_seed_circle_batch'):          # absent from a CLH_LIB build older than the circles of a batch: circles() raises there
            L.clh_seed_circle_batch.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(ChainOpts), C.POINTER(LinkOpts), C.POINTER(JunctionOpts),
                                                C.POINTER(Splice), C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.c_void_p]
            L.clh_seed_circle_table_fetch.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
        L.clh_band_plan_create.restype = C.c_void_p
        L.clh_band_plan_create.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(BandOpts)]
        L.clh_band_plan_destroy.restype = None
        L.clh_band_plan_destroy.argtypes = [C.c_void_p]
        L.clh_band_plan_run.argtypes = [C.c_void_p, C.c_void_p]
        L.clh_band_plan_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
        L.clh_band_plan_timing.argtypes = [C.c_void_p, C.c_void_p]
        L.clh_band_plan_info.argtypes = [C.c_void_p, C.c_void_p]
        L.clh_band_batch.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(BandOpts), C.c_void_p,
                                     C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
        L.clh_poa_batch.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p]
        L.clh_ccs_results_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.clh_ccs_plan_info.argtypes = [C.c_void_p, C.c_void_p]
        L.clh_ccs_plan_stats.argtypes = [C.c_void_p, C.c_void_p]
        L.clh_poa_last_stats.argtypes = [C.c_void_p, C.c_void_p]
        L.clh_plan_set_profiling.argtypes = [C.c_void_p, C.c_int]
        L.clh_plan_segments.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.clh_plan_timing.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        L.clh_plan_traceback_counts.argtypes = [C.c_void_p, C.c_void_p]
        L.clh_plan_prefilter_stats.argtypes = [C.c_void_p, C.c_void_p]
        L.clh_plan_prefilter_timing.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.clh_plan_set_refs_bytes.argtypes = [C.c_void_p, C.c_int64]
        _lib = L
    return _lib


def fastx_index(in_path, is_fastq, every=4096):
    """(records, [byte offset of record 0, every, 2 every, ...]) of a FASTA/FASTQ file; no offsets for a gzip file (host only)"""
    n = C.c_int64(0); no = C.c_int64(0)
    L = lib()
    L.clh_fastx_index.argtypes = [C.c_char_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    cap = max(16, os.path.getsize(in_path) // max(1, 20 * every) + 16)
    off = np.zeros(cap, dtype=np.int64)
    if L.clh_fastx_index(os.fsencode(in_path), int(bool(is_fastq)), int(every), C.byref(n), off.ctypes.data, cap, C.byref(no)) != 0:
        raise ClhError('clh_fastx_index failed for %s' % in_path)
    return int(n.value), [int(x) for x in off[:no.value]]


def fastx_count(in_path, is_fastq):
    """records of a FASTA/FASTQ(.gz) file as find_ccs_reads' loop counts them (host only, no GPU)"""
    n = C.c_int64(0)
    if lib().clh_fastx_count(os.fsencode(in_path), int(bool(is_fastq)), C.byref(n)) != 0:
        raise ClhError('clh_fastx_count failed for %s' % in_path)
    return int(n.value)


def last_error():
    return lib().clh_last_error().decode()


def _check(rc, what):
    """raise ClhError('<what> failed (<rc>): <last error>') for a non-zero return code of libclh"""
    if rc != 0:
        raise ClhError('%s failed (%d): %s' % (what, rc, last_error()))


class _Handle(object):
    """A libclh object that belongs to a Context (a plan, a resident genome).  close() destroys it once, and not after the context
    has closed: clh_destroy has given back everything the context's objects held."""
    _destroy = None         # name of the libclh function that destroys the handle

    def __init__(self, ctx):
        self.ctx, self._h = ctx, None

    def close(self):
        h, self._h = getattr(self, '_h', None), None
        if h and getattr(self.ctx, '_h', None):
            getattr(lib(), self._destroy)(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _timing(self, name):
        """HIP-event milliseconds of the last run, from the libclh function `name`(handle, float*)"""
        ms = C.c_float(0)
        _check(getattr(lib(), name)(self._h, C.byref(ms)), name)
        return float(ms.value)


_LUT = np.full(256, 4, dtype=np.int8)
for _c, _v in zip('ACGTN', range(5)):
    _LUT[ord(_c)] = _v
    _LUT[ord(_c.lower())] = _v


def encode(seq):
    """ASCII -> int8 codes, the mapping of ssw_wrap.py:50,243-250 (vectorised; the reference loops per base)."""
    if isinstance(seq, str):
        seq = seq.encode('latin-1')
    return _LUT[np.frombuffer(seq, dtype=np.uint8)]


def pack_raw(seqs):
    """list of str / bytes -> (the letters as they are, one byte each, int64 offsets[n+1]): the partial-order aligner compares
    letters for equality only (spoa's alphabet is the set of raw characters)"""
    arrs = [np.frombuffer(s.encode('latin-1') if isinstance(s, str) else bytes(s), dtype=np.int8) for s in seqs]
    off = np.zeros(len(arrs) + 1, dtype=np.int64)
    if arrs:
        np.cumsum([len(a) for a in arrs], out=off[1:])
    data = np.concatenate(arrs) if arrs else np.zeros(0, dtype=np.int8)
    return np.ascontiguousarray(data, dtype=np.int8), off


def score_matrix(match, mismatch):
    """ssw_wrap.py:146-159: match on the diagonal, -mismatch elsewhere, 0 for N."""
    m = np.full((5, 5), -int(mismatch), dtype=np.int8)
    np.fill_diagonal(m, int(match))
    m[4, :] = 0
    m[:, 4] = 0
    return np.ascontiguousarray(m.reshape(-1))


def pack(seqs):
    """list of int8 arrays / str -> (packed int8 array, int64 offsets[n+1])"""
    arrs = [encode(s) if isinstance(s, (str, bytes)) else np.asarray(s, dtype=np.int8) for s in seqs]
    off = np.zeros(len(arrs) + 1, dtype=np.int64)
    if arrs:
        np.cumsum([len(a) for a in arrs], out=off[1:])
    data = np.concatenate(arrs) if arrs else np.zeros(0, dtype=np.int8)
    return np.ascontiguousarray(data, dtype=np.int8), off


def pack_text(seqs):
    """pack() for a list of str only, encoded in one pass over their concatenation (a clip batch is thousands of short strings)"""
    blob = ''.join(seqs).encode('latin-1')
    off = np.zeros(len(seqs) + 1, dtype=np.int64)
    if seqs:
        np.cumsum([len(s) for s in seqs], out=off[1:])
    return np.ascontiguousarray(_LUT[np.frombuffer(blob, dtype=np.uint8)], dtype=np.int8), off


def _torch_first():
    """torch ships its own HIP runtime; when a process uses both, torch's must open the device before libclh's does
    (the other order leaves torch with "No HIP GPUs are available").  Only acts when the caller already imported torch."""
    t = sys.modules.get('torch')
    if t is not None and t.cuda.is_available() and not t.cuda.is_initialized():
        t.cuda.init()


class Context(object):
    """One per (process, GPU)."""

    def __init__(self, device=0):
        global _gpu_used
        L = lib()
        _torch_first()
        self._h = L.clh_create(int(device))
        if not self._h:
            raise HipUnavailable('clh_create(%d) failed: %s (there is no CPU fallback)' % (device, last_error()))
        _gpu_used = True
        self.device = int(device)

    def close(self):
        if getattr(self, '_h', None):
            lib().clh_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _opts(self, mat, gap_open, gap_extend, flag, score_size, want_score2, want_cigar, filters=0, filterd=0):
        mat = np.ascontiguousarray(mat, dtype=np.int8)
        o = SswOpts()
        o.mat = mat.ctypes.data
        o.n_mat = int(round(len(mat) ** 0.5))
        o.gap_open, o.gap_extend, o.flag, o.score_size = int(gap_open), int(gap_extend), int(flag), int(score_size)
        o.filters, o.filterd, o.want_score2, o.want_cigar = int(filters), int(filterd), int(want_score2), int(want_cigar)
        return o, mat

    def ssw_batch(self, reads, read_off, refs, ref_off, mat, gap_open, gap_extend, flag=1, score_size=2,
                  want_score2=True, want_cigar=True, mask_len=None, filters=0, filterd=0):
        """Host arrays in, (rows: structured array, cigars: uint32 array) out.  flag / filters / filterd as ssw_align
        takes them (ssw.h:95-111: bit 1 score filter, bit 2 distance filter, bit 3 = bit 0 for the begin positions)."""
        L = lib()
        reads = np.ascontiguousarray(reads, dtype=np.int8)
        refs = np.ascontiguousarray(refs, dtype=np.int8)
        read_off = np.ascontiguousarray(read_off, dtype=np.int64)
        ref_off = np.ascontiguousarray(ref_off, dtype=np.int64)
        n = len(read_off) - 1
        o, _keep = self._opts(mat, gap_open, gap_extend, flag, score_size, want_score2, want_cigar, filters, filterd)
        out = np.zeros(n, dtype=ALIGN_DTYPE)
        cap = int(2 * (read_off[-1] if n else 0) + 2 * n + 8) if want_cigar else 1
        cig = np.empty(cap, dtype=np.uint32)     # worst-case capacity; only the used prefix is written
        used = C.c_int64(0)
        ml = None
        if mask_len is not None:
            ml = np.ascontiguousarray(mask_len, dtype=np.int32)
        _check(L.clh_ssw_batch(self._h, n, reads.ctypes.data, read_off.ctypes.data, refs.ctypes.data, ref_off.ctypes.data,
                               ml.ctypes.data if ml is not None else None, C.byref(o), out.ctypes.data,
                               cig.ctypes.data if want_cigar else None, cap, C.byref(used)), 'clh_ssw_batch')
        return out, cig[:used.value]

    def ccs_batch(self, reads, read_off):
        """find_consensus for a batch: -> (rows CCS_DTYPE[n], segs int32[n, 65, 2], ccs int8 packed like reads)"""
        reads = np.ascontiguousarray(reads, dtype=np.int8)
        read_off = np.ascontiguousarray(read_off, dtype=np.int64)
        n = len(read_off) - 1
        out = np.zeros(n, dtype=CCS_DTYPE)
        segs = np.zeros((n, CCS_SEG_CAP, 2), dtype=np.int32)
        ccs = np.zeros(max(1, len(reads)), dtype=np.int8)
        _check(lib().clh_ccs_batch(self._h, n, reads.ctypes.data, read_off.ctypes.data, out.ctypes.data, segs.ctypes.data, ccs.ctypes.data), 'clh_ccs_batch')
        return out, segs, ccs

    def poa_batch(self, seqs, seq_off, group_off, algorithm=0, scores=(10, -4, -8, -2, -24, -1), min_coverage=0, genmsa=False,
                  with_scores=False, raw=False):
        """spoa.poa per group of sequences: -> list of consensus str, or list of (consensus, msa rows[, end-cell scores of
        the first 65 sequences]) with genmsa / with_scores.  The letters of `seqs` are bytes compared for equality only;
        raw=False reads them as the codes 0..4 of `encode` and writes ACGTN, raw=True hands them through as characters
        (`pack_raw`).  Raises ClhError when a group has no consensus (a node with more than 48
        in-edges, more than 8 different letters in a column) or the scores are outside what the kernel honours."""
        seqs = np.ascontiguousarray(seqs, dtype=np.int8)
        seq_off = np.ascontiguousarray(seq_off, dtype=np.int64)
        group_off = np.ascontiguousarray(group_off, dtype=np.int64)
        ng = len(group_off) - 1
        lens = np.zeros(ng, dtype=np.int32)
        out = np.zeros(max(1, len(seqs)), dtype=np.int8)
        opts = np.array([algorithm] + [int(x) for x in scores] + [min_coverage], dtype=np.int32)
        col = np.zeros(max(1, len(seqs)), dtype=np.int32) if genmsa else None
        ncols = np.zeros(max(1, ng), dtype=np.int32) if genmsa else None
        asc = np.zeros((max(1, ng), CCS_SEG_CAP), dtype=np.int32) if with_scores else None
        _check(lib().clh_poa_batch(self._h, ng, seqs.ctypes.data, seq_off.ctypes.data, group_off.ctypes.data, opts.ctypes.data,
                                   lens.ctypes.data, out.ctypes.data, col.ctypes.data if genmsa else None,
                                   ncols.ctypes.data if genmsa else None, asc.ctypes.data if with_scores else None), 'clh_poa_batch')
        bases = np.frombuffer(b'ACGTN', dtype=np.uint8)
        res = []
        for k in range(ng):
            if lens[k] < 0:
                raise ClhError('poa: no consensus for group %d (status %d: 1 workspace, 2 graph limits -- more than 48 in-edges, more than 8 '
                               'letters in a column or 65000 nodes, 3 output, 4 (unused since round 4), 5 back-track guard, 6 a cell left the '
                               '16-bit score range, 7 an alignment without a base: spoa throws)' % (k, -1 - int(lens[k])))
            o = int(seq_off[group_off[k]])
            text = (lambda a: a.view(np.uint8).tobytes().decode('latin-1')) if raw else (lambda a: bases[np.minimum(a, 4)].tobytes().decode())
            cons = text(out[o:o + int(lens[k])])
            if not genmsa and not with_scores:
                res.append(cons)
                continue
            rows = []
            if genmsa:
                for i in range(int(group_off[k]), int(group_off[k + 1])):
                    row = np.full(int(ncols[k]), ord('-'), dtype=np.uint8)
                    a, b = int(seq_off[i]), int(seq_off[i + 1])
                    row[col[a:b]] = seqs[a:b].view(np.uint8) if raw else bases[np.minimum(seqs[a:b], 4)]
                    rows.append(row.tobytes().decode('latin-1'))
            item = (cons, rows)
            if with_scores:
                item = item + ([int(x) for x in asc[k, :min(CCS_SEG_CAP, int(group_off[k + 1] - group_off[k]))]],)
            res.append(item)
        return res

    def poa_last_stats(self):
        """statistics of the last poa_batch (see CcsPlan.stats)"""
        out = np.zeros(16, dtype=np.int64)
        _check(lib().clh_poa_last_stats(self._h, out.ctypes.data), 'clh_poa_last_stats')
        return {'dp_cells': int(out[0]), 'dp_row_steps': int(out[1]), 'band_misses': int(out[2]), 'dropped': {k: int(out[2 + k]) for k in range(1, 8) if out[2 + k]}}

    def edit_distance_batch(self, xs, ys):
        """Unit-cost edit distance of the pairs (xs[k], ys[k]) (str or bytes) -> int32 array.  K4 through the C ABI."""
        n = len(xs)
        if n != len(ys):
            raise ValueError('edit_distance_batch: the two lists differ in length')
        ba = [x.encode() if isinstance(x, str) else bytes(x) for x in xs]
        bb = [y.encode() if isinstance(y, str) else bytes(y) for y in ys]
        a_off = np.zeros(n + 1, dtype=np.int64); b_off = np.zeros(n + 1, dtype=np.int64)
        if n:
            a_off[1:] = np.cumsum([len(x) for x in ba]); b_off[1:] = np.cumsum([len(y) for y in bb])
        a = np.frombuffer(b''.join(ba) + b'\0', dtype=np.uint8)
        b = np.frombuffer(b''.join(bb) + b'\0', dtype=np.uint8)
        out = np.zeros(n, dtype=np.int32)
        _check(lib().clh_edit_distance_batch(self._h, n, a.ctypes.data, a_off.ctypes.data, b.ctypes.data, b_off.ctypes.data, out.ctypes.data), 'clh_edit_distance_batch')
        return out

    def edit_plan(self, xs, ys):
        return EditPlan(self, xs, ys)

    def edit_matrix_batch(self, groups, hpc=False):
        """Every pair i < j of every group (a list of lists of str or bytes) in one call, the strings uploaded once -> per group
        (condensed int32 distances in np.triu_indices(n, 1) order, int32 lengths); with hpc=True the strings are homopolymer-
        compressed on the device first and each group's tuple ends with the compressed strings.  See EditMatrixPlan."""
        pk = _EditMatrixInput(groups)
        dist = np.zeros(pk.npairs, dtype=np.int32); lens = np.zeros(pk.nseq, dtype=np.int32)
        out = np.zeros(pk.data.size, dtype=np.uint8) if hpc else None
        _check(lib().clh_edit_matrix_batch(self._h, pk.nseq, pk.data.ctypes.data, pk.off.ctypes.data, len(groups), pk.goff.ctypes.data, 1 if hpc else 0,
                                           dist.ctypes.data, dist.size, lens.ctypes.data, out.ctypes.data if hpc else None, out.size if hpc else 0),
               'clh_edit_matrix_batch')
        return pk.split(dist, lens, out)

    def edit_matrix_plan(self, groups, hpc=False):
        return EditMatrixPlan(self, groups, hpc)

    def hpc_compress_batch(self, seqs):
        """Homopolymer compression of every string (str or bytes) on the device, no distances: the same call without groups."""
        pk = _EditMatrixInput([seqs])
        lens = np.zeros(pk.nseq, dtype=np.int32); out = np.zeros(pk.data.size, dtype=np.uint8)
        _check(lib().clh_edit_matrix_batch(self._h, pk.nseq, pk.data.ctypes.data, pk.off.ctypes.data, 0, None, 1, None, 0, lens.ctypes.data,
                                           out.ctypes.data, out.size), 'clh_edit_matrix_batch')
        return pk.split(np.zeros(0, dtype=np.int32), lens, out)[0][2]

    def edit_align_batch(self, queries, targets, mode='NW', task='distance', k=-1, equalities=(), workspace_bytes=0):
        """edlib.align of the pairs (queries[k], targets[k]) (str or bytes) through K4m / K4t -> (rows EDIT_ALIGN_DTYPE,
        locs int32[.., 2] of (start, end), cigar uint32 BAM ops).  equalities: pairs of letters that also match."""
        plan = EditAlignPlan(self, queries, targets, mode, task, k, equalities, workspace_bytes)
        try:
            plan.run()
            return plan.fetch()
        finally:
            plan.close()

    def edit_align_plan(self, queries, targets, mode='NW', task='distance', k=-1, equalities=(), workspace_bytes=0):
        return EditAlignPlan(self, queries, targets, mode, task, k, equalities, workspace_bytes)

    def edit_search_batch(self, probes, texts, k=-1, equalities=()):
        """Every probe (str or bytes, at most 64 letters) against every text, HW with locations, through K4s -> EDIT_SEARCH_DTYPE
        array [len(texts), len(probes)].  See EditSearchPlan."""
        plan = EditSearchPlan(self, probes, texts, k, equalities)
        try:
            plan.run()
            return plan.fetch()
        finally:
            plan.close()

    def edit_search_plan(self, probes, texts, k=-1, equalities=()):
        return EditSearchPlan(self, probes, texts, k, equalities)

    def ends_batch(self, queries, query_off, refs, ref_off, mat, gap_open, gap_extend, mode='global', want_cigar=True, workspace_bytes=0,
                   gap_open2=None, gap_extend2=None, splice=None, strand=None, traceback='stored', windows=None):
        """End-anchored affine-gap alignment of the pairs (query k, reference k), packed codes and offsets as ssw_batch takes them,
        through K1g -> (rows ENDS_DTYPE, cigars uint32 packed ops).  See EndsPlan."""
        plan = EndsPlan(self, queries, query_off, refs, ref_off, mat, gap_open, gap_extend, mode, want_cigar, workspace_bytes, gap_open2, gap_extend2,
                        splice, strand, traceback, windows)
        try:
            plan.run()
            return plan.fetch()
        finally:
            plan.close()

    def ends_plan(self, queries, query_off, refs, ref_off, mat, gap_open, gap_extend, mode='global', want_cigar=True, workspace_bytes=0,
                  gap_open2=None, gap_extend2=None, splice=None, strand=None, traceback='stored', windows=None):
        return EndsPlan(self, queries, query_off, refs, ref_off, mat, gap_open, gap_extend, mode, want_cigar, workspace_bytes, gap_open2, gap_extend2,
                        splice, strand, traceback, windows)

    def band_batch(self, queries, query_off, refs, ref_off, mat, gap_open, gap_extend, band, mode='global', diagonals=None, want_cigar=True,
                   workspace_bytes=0, gap_open2=None, gap_extend2=None, windows=None):
        """Banded end-anchored alignment of the pairs (query k, reference k) through K1gb: the programme of ends_batch over the
        diagonals within `band` of the corner diagonals, or of diagonals[k] -> (rows BAND_DTYPE, cigars uint32 packed ops).  See BandPlan."""
        plan = BandPlan(self, queries, query_off, refs, ref_off, mat, gap_open, gap_extend, band, mode, diagonals, want_cigar, workspace_bytes,
                        gap_open2, gap_extend2, windows)
        try:
            plan.run()
            return plan.fetch()
        finally:
            plan.close()

    def band_plan(self, queries, query_off, refs, ref_off, mat, gap_open, gap_extend, band, mode='global', diagonals=None, want_cigar=True,
                  workspace_bytes=0, gap_open2=None, gap_extend2=None, windows=None):
        return BandPlan(self, queries, query_off, refs, ref_off, mat, gap_open, gap_extend, band, mode, diagonals, want_cigar, workspace_bytes,
                        gap_open2, gap_extend2, windows)

    def ccs_file(self, in_path, is_fastq, ccs_fa_path, raw_fa_path, batch_reads=0, first_record=0, max_records=-1, byte_offset=0):
        """Stage 1 from file to file in native code -> (total_reads, reads_with_consensus, reads_too_long); with
        first_record / max_records for one rank's contiguous shard of the records, counted from `byte_offset` (the first byte of a
        record, `fastx_index`).  Reads that a limit of the kernel left without a consensus are counted in self.capacity_dropped
        (and logged by find_ccs_reads)."""
        st = (C.c_int64 * 4)()
        L = lib()
        L.clh_ccs_file_at.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_char_p, C.c_char_p, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_void_p]
        _check(L.clh_ccs_file_at(self._h, os.fsencode(in_path), int(bool(is_fastq)), os.fsencode(ccs_fa_path), os.fsencode(raw_fa_path),
                                 int(batch_reads), int(byte_offset), int(first_record), int(max_records), C.byref(st)), 'clh_ccs_file')
        self.capacity_dropped = getattr(self, 'capacity_dropped', 0) + int(st[3])
        self.last_capacity_dropped = int(st[3])
        return int(st[0]), int(st[1]), int(st[2])

    @staticmethod
    def release_file_buffers():
        """give back the host and device buffers the file stage (ccs_file) keeps between calls"""
        lib().clh_ccs_file_release_buffers()

    def ccs_plan(self, read_off):
        return CcsPlan(self, read_off)

    def plan(self, read_off, ref_off, mat, gap_open, gap_extend, flag=1, score_size=2, want_score2=True,
             want_cigar=True, mask_len=None):
        return Plan(self, read_off, ref_off, mat, gap_open, gap_extend, flag, score_size, want_score2, want_cigar, mask_len)


def _pack_bytes(items):
    bs = [x.encode() if isinstance(x, str) else bytes(x) for x in items]
    off = np.zeros(len(bs) + 1, dtype=np.int64)
    if bs:
        off[1:] = np.cumsum([len(x) for x in bs])
    return np.frombuffer(b''.join(bs) + b'\0', dtype=np.uint8), off


class EditPlan(_Handle):
    """Pairs of strings resident on the GPU: run() the edit distances any number of times, fetch() the int32 array."""
    _destroy = 'clh_edit_plan_destroy'

    def __init__(self, ctx, xs, ys):
        _Handle.__init__(self, ctx)
        if len(xs) != len(ys):
            raise ValueError('EditPlan: the two lists differ in length')
        self.n = len(xs)
        a, a_off = _pack_bytes(xs)
        b, b_off = _pack_bytes(ys)
        self._h = lib().clh_edit_plan_create(ctx._h, self.n, a.ctypes.data, a_off.ctypes.data, b.ctypes.data, b_off.ctypes.data)
        if not self._h:
            raise ClhError('clh_edit_plan_create failed: %s' % last_error())

    def run(self, stream=0):
        _check(lib().clh_edit_plan_run(self._h, C.c_void_p(stream)), 'clh_edit_plan_run')

    def fetch(self):
        out = np.zeros(self.n, dtype=np.int32)
        _check(lib().clh_edit_plan_fetch(self._h, out.ctypes.data), 'clh_edit_plan_fetch')
        return out

    def timing(self):
        return self._timing('clh_edit_plan_timing')


class _EditMatrixInput(object):
    """groups (a list of lists of str or bytes) packed for clh_edit_matrix_*: every string once, groups as runs of strings"""

    def __init__(self, groups):
        flat = [s for g in groups for s in g]
        self.is_str = [isinstance(s, str) for s in flat]
        self.data, self.off = _pack_bytes(flat)
        self.nseq = len(flat)
        self.goff = np.zeros(len(groups) + 1, dtype=np.int64)
        if groups:
            self.goff[1:] = np.cumsum([len(g) for g in groups])
        m = np.diff(self.goff)
        self.pair_off = np.concatenate(([0], np.cumsum(m * (m - 1) // 2))).astype(np.int64)
        self.npairs = int(self.pair_off[-1])

    def split(self, dist, lens, hpc):
        """the flat outputs of a fetch -> per group (distances, lengths[, compressed strings])"""
        res = []
        if hpc is not None:
            at = np.concatenate(([0], np.cumsum(lens, dtype=np.int64)))
            blob = hpc.tobytes()
        for g in range(len(self.goff) - 1):
            a, b = int(self.goff[g]), int(self.goff[g + 1])
            item = (dist[self.pair_off[g]:self.pair_off[g + 1]], lens[a:b])
            if hpc is not None:
                strs = [blob[at[s]:at[s + 1]] for s in range(a, b)]
                item += ([x.decode() if self.is_str[s] else x for s, x in zip(range(a, b), strs)],)
            res.append(item)
        return res


class EditMatrixPlan(_Handle):
    """Groups of strings resident on the GPU (each string uploaded once): run() computes every group's condensed edit-distance
    matrix any number of times -- compression (hpc=True), the pair tasks and K4, all on the device -- fetch() returns per group
    (int32 distances in np.triu_indices(n, 1) order, int32 lengths the distances were computed on[, the compressed strings])."""
    _destroy = 'clh_edit_matrix_plan_destroy'

    def __init__(self, ctx, groups, hpc=False):
        _Handle.__init__(self, ctx)
        self.hpc = bool(hpc)
        self._in = pk = _EditMatrixInput(groups)
        self.ngroups, self.npairs = len(groups), pk.npairs
        self._h = lib().clh_edit_matrix_plan_create(ctx._h, pk.nseq, pk.data.ctypes.data, pk.off.ctypes.data, self.ngroups, pk.goff.ctypes.data, int(self.hpc))
        if not self._h:
            raise ClhError('clh_edit_matrix_plan_create failed: %s' % last_error())

    def run(self, stream=0):
        _check(lib().clh_edit_matrix_plan_run(self._h, C.c_void_p(stream)), 'clh_edit_matrix_plan_run')

    def sizes(self):
        """(pairs, bytes of the strings the distances were computed on) of the last run"""
        n = C.c_int64(0); b = C.c_int64(0)
        _check(lib().clh_edit_matrix_plan_sizes(self._h, C.byref(n), C.byref(b)), 'clh_edit_matrix_plan_sizes')
        return int(n.value), int(b.value)

    def fetch(self):
        pk = self._in
        dist = np.zeros(pk.npairs, dtype=np.int32); lens = np.zeros(pk.nseq, dtype=np.int32)
        out = np.zeros(self.sizes()[1], dtype=np.uint8) if self.hpc else None
        _check(lib().clh_edit_matrix_plan_fetch(self._h, dist.ctypes.data, dist.size, lens.ctypes.data, out.ctypes.data if self.hpc else None,
                                                out.size if self.hpc else 0), 'clh_edit_matrix_plan_fetch')
        return pk.split(dist, lens, out)

    def timing(self):
        """HIP-event milliseconds of the last run: compression + task build + K4"""
        return self._timing('clh_edit_matrix_plan_timing')


def _letter(c):
    if isinstance(c, int):
        return c
    b = c.encode('latin-1') if isinstance(c, str) else bytes(c)
    if len(b) != 1:
        raise ValueError('an equality pairs two single letters, got %r' % (c,))
    return b[0]


class EditAlignPlan(_Handle):
    """Pairs resident on the GPU for edlib.align's modes: run() any number of times, fetch() (rows, locs, cigar)."""
    _destroy = 'clh_edit_align_plan_destroy'

    def __init__(self, ctx, queries, targets, mode='NW', task='distance', k=-1, equalities=(), workspace_bytes=0):
        _Handle.__init__(self, ctx)
        if len(queries) != len(targets):
            raise ValueError('EditAlignPlan: the two lists differ in length')
        if mode not in EA_MODES:
            raise ValueError('mode must be one of NW, SHW, HW, got %r' % (mode,))
        if task not in EA_TASKS:
            raise ValueError('task must be one of distance, locations, path, got %r' % (task,))
        self.n = len(queries)
        q, q_off = _pack_bytes(queries)
        t, t_off = _pack_bytes(targets)
        eq = np.array([[_letter(a), _letter(b)] for a, b in (equalities or ())], dtype=np.uint8).reshape(-1)
        self._eq = np.ascontiguousarray(np.concatenate([eq, np.zeros(2, dtype=np.uint8)]))
        opts = EditAlignOpts(EA_MODES[mode], EA_TASKS[task], int(k), len(eq) // 2, self._eq.ctypes.data, int(workspace_bytes))
        self._h = lib().clh_edit_align_plan_create(ctx._h, self.n, q.ctypes.data, q_off.ctypes.data, t.ctypes.data, t_off.ctypes.data,
                                                   C.byref(opts))
        if not self._h:
            raise ClhError('clh_edit_align_plan_create failed: %s' % last_error())
        lc, cc = C.c_int64(0), C.c_int64(0)
        lib().clh_edit_align_plan_caps(self._h, C.byref(lc), C.byref(cc))
        self._caps = (int(lc.value), int(cc.value))

    def run(self, stream=0):
        _check(lib().clh_edit_align_plan_run(self._h, C.c_void_p(stream)), 'clh_edit_align_plan_run')

    def fetch(self):
        rows = np.zeros(self.n, dtype=EDIT_ALIGN_DTYPE)
        locs = np.zeros((max(self._caps[0], 1), 2), dtype=np.int32)
        cig = np.zeros(max(self._caps[1], 1), dtype=np.uint32)
        lu, cu = C.c_int64(0), C.c_int64(0)
        _check(lib().clh_edit_align_plan_fetch(self._h, rows.ctypes.data, locs.ctypes.data, self._caps[0], C.byref(lu), cig.ctypes.data,
                                               self._caps[1], C.byref(cu)), 'clh_edit_align_plan_fetch')
        return rows, locs[:lu.value].copy(), cig[:cu.value].copy()

    def timing(self):
        return self._timing('clh_edit_align_plan_timing')


class EditSearchPlan(_Handle):
    """Probes and texts resident on the GPU (each uploaded once) for the cross product of HW searches: run() any number of times,
    fetch() the EDIT_SEARCH_DTYPE array [len(texts), len(probes)] -- per cell the distance, (start, end) of the first location,
    the end of the last one and their number, as edlib.align(probe, text, mode='HW', task='locations') states them."""
    _destroy = 'clh_edit_search_plan_destroy'

    def __init__(self, ctx, probes, texts, k=-1, equalities=()):
        _Handle.__init__(self, ctx)
        self.ntext, self.nprobe = len(texts), len(probes)
        t, t_off = _pack_bytes(texts)
        q, q_off = _pack_bytes(probes)
        eq = np.array([[_letter(a), _letter(b)] for a, b in (equalities or ())], dtype=np.uint8).reshape(-1)
        self._eq = np.ascontiguousarray(np.concatenate([eq, np.zeros(2, dtype=np.uint8)]))
        opts = EditSearchOpts(int(k), len(eq) // 2, self._eq.ctypes.data)
        self._h = lib().clh_edit_search_plan_create(ctx._h, self.ntext, t.ctypes.data, t_off.ctypes.data, self.nprobe, q.ctypes.data,
                                                    q_off.ctypes.data, C.byref(opts))
        if not self._h:
            raise ClhError('clh_edit_search_plan_create failed: %s' % last_error())

    def run(self, stream=0):
        _check(lib().clh_edit_search_plan_run(self._h, C.c_void_p(stream)), 'clh_edit_search_plan_run')

    def fetch(self):
        rows = np.zeros((self.ntext, self.nprobe), dtype=EDIT_SEARCH_DTYPE)
        _check(lib().clh_edit_search_plan_fetch(self._h, rows.ctypes.data, rows.size), 'clh_edit_search_plan_fetch')
        return rows

    def timing(self):
        return self._timing('clh_edit_search_plan_timing')

    def info(self):
        """the geometry of the kernel: columns a lane owns per round (seg), columns of a wave's round, columns one wave walks before a
        text is split over several waves (chunk); and of this plan: chunks, split texts, probes per word width"""
        out = (C.c_int64 * 8)()
        _check(lib().clh_edit_search_plan_info(self._h, out), 'clh_edit_search_plan_info')
        return {'seg': int(out[0]), 'round': int(out[1]), 'chunk': int(out[2]), 'texts_per_launch': int(out[3]), 'chunks': int(out[4]),
                'split_texts': int(out[5]), 'probes32': int(out[6]), 'probes64': int(out[7])}


class _PairsPlan(_Handle):
    """What EndsPlan and BandPlan share: the inputs as libclh takes them, run(), fetch() and timing().  A subclass names its C
    prefix (`_c`, as in clh_<_c>_plan_run) and the dtype of its rows."""
    _c = _dtype = None

    def _inputs(self, queries, query_off, refs, ref_off, mat, want_cigar, diagonals=None, windows=None):
        """-> (codes and offsets as contiguous arrays, the flat int8 matrix, its edge, the diagonals as int32 or None); sets n and
        want_cigar.  With `windows` = (Genome, offsets, lengths, flags) the references are windows of a resident genome instead of
        refs and ref_off, which must then be None: r is the Genome and r_off the three arrays (int64, int32, uint8), kept alive here"""
        who = type(self).__name__
        q = np.ascontiguousarray(queries, dtype=np.int8)
        q_off = np.ascontiguousarray(query_off, dtype=np.int64)
        if windows is not None:
            if refs is not None or ref_off is not None:
                raise ValueError('%s: the references are either refs and ref_off or windows, not both' % who)
            if not hasattr(lib(), 'clh_ends_plan_create_windows'):
                raise ClhError('%s: this libclh.so is older than pair plans on genome windows' % who)
            genome, off, ln, flags = windows
            if not isinstance(genome, Genome) or not genome._h:
                raise ValueError('%s: windows = (hip.Genome, offsets, lengths, flags)' % who)
            if genome.ctx is not self.ctx:
                raise ValueError('%s: the genome lives on another context' % who)
            r = genome
            r_off = (np.ascontiguousarray(off, dtype=np.int64), np.ascontiguousarray(ln, dtype=np.int32), np.ascontiguousarray(flags, dtype=np.uint8))
            if len(q_off) < 1 or any(a.shape != (len(q_off) - 1,) for a in r_off):
                raise ValueError('%s: %d query offsets need %d window offsets, lengths and flags' % (who, len(q_off), len(q_off) - 1))
        else:
            if refs is None or ref_off is None:
                raise ValueError('%s: the references are refs and ref_off, or windows' % who)
            r = np.ascontiguousarray(refs, dtype=np.int8)
            r_off = np.ascontiguousarray(ref_off, dtype=np.int64)
            if len(q_off) != len(r_off) or len(q_off) < 1:
                raise ValueError('%s: the two offset tables differ in length' % who)
        self.n = len(q_off) - 1
        self.want_cigar = bool(want_cigar)
        diag = None
        if diagonals is not None:
            diag = np.ascontiguousarray(diagonals, dtype=np.int32)
            if diag.shape != (self.n,):
                raise ValueError('%s: %d diagonals for %d pairs' % (who, diag.size, self.n))
        mat = np.ascontiguousarray(mat, dtype=np.int8).reshape(-1)
        n_mat = int(round(len(mat) ** 0.5))
        if n_mat * n_mat != len(mat):
            raise ValueError('%s: the substitution matrix is not square' % who)
        return q, q_off, r, r_off, mat, n_mat, diag

    def run(self, stream=0):
        name = 'clh_%s_plan_run' % self._c
        _check(getattr(lib(), name)(self._h, C.c_void_p(stream)), name)

    def fetch(self):
        name = 'clh_%s_plan_fetch' % self._c
        rows = np.zeros(self.n, dtype=self._dtype)
        cap = self.info()['cigar_cap'] if self.want_cigar else 0
        cig = np.empty(max(cap, 1), dtype=np.uint32)     # worst-case capacity; only the used prefix is written
        used = C.c_int64(0)
        _check(getattr(lib(), name)(self._h, rows.ctypes.data, cig.ctypes.data if self.want_cigar else None, cap, C.byref(used)), name)
        return rows, cig[:used.value].copy()

    def timing(self):
        """HIP-event milliseconds of the last run: the score kernels (of every class, where there are classes), and with CIGARs
        the walks, of every share of the batch"""
        return self._timing('clh_%s_plan_timing' % self._c)

    def gather_timing(self):
        """a plan made with windows=: (HIP-event milliseconds of the gather that filled its reference buffer, letters moved)"""
        name = 'clh_%s_plan_gather_timing' % self._c
        ms, letters = C.c_float(0), C.c_int64(0)
        _check(getattr(lib(), name)(self._h, C.byref(ms), C.byref(letters)), name)
        return float(ms.value), int(letters.value)


class EndsPlan(_PairsPlan):
    """Pairs resident on the GPU (codes uploaded once) for the end-anchored modes of K1g -- 'global', 'semiglobal' (the whole query in
    any stretch of the reference), 'overlap' (end gaps free on both sequences) -- and the start-anchored ones, pinned at (0, 0) and
    free at the far end: 'prefix' (the whole query against a prefix of the reference), 'extend' (a prefix of the query against a
    prefix of the reference, the best cell of the whole matrix; score >= 0): run() any number of times, fetch() (rows ENDS_DTYPE,
    cigars uint32).  Scores are int32 and may be negative; a span without a letter has end == begin - 1; without want_cigar no walk
    back is made and a begin the mode does not fix is -1 (include/ciri_long_hip.h).  With gap_open2 and gap_extend2 a gap of k
    letters costs the smaller of gap_open + (k - 1) gap_extend and gap_open2 + (k - 1) gap_extend2 (0 <= gap_extend2 <= gap_extend
    <= gap_open <= gap_open2; clh_ends_plan_create_gap2), and the stored decisions take a byte per cell instead of half a byte.
    With `splice` (a Splice, see splice_of) a run of skipped reference letters costs the smaller of a deletion and an intron, whose
    cost is intron_open plus the donor and acceptor costs of the dinucleotides at its ends on the pair's strand (`strand`: +1 / -1 per
    pair, None for all +1; clh_ends_plan_create_spliced); CIGARs then hold op N (3), a byte per cell is stored, the matrix must be the
    DNA match / mismatch one, and two-piece gap costs together with introns are not built.
    traceback names the route to the CIGARs: 'stored' keeps the decisions of every cell of a pair (half a byte or a byte per cell of
    m x n) in the workspace; 'recompute' keeps the last column of every chunk of 512 reference columns, computes the decisions again
    one chunk at a time and resumes the walk chunk after chunk (CLH_ENDS_CIGAR_RECOMPUTE): the same rows and CIGARs, bit for bit, from
    a 32nd to a 43rd of the memory per chunk, at the price of computing the cells the walk can reach twice.  It pays from about four
    chunks on; no routing is made between the two.
    windows=(genome, offsets, lengths, flags) stands for refs and ref_off (both None then; giving both is a ValueError): reference k
    is lengths[k] bases of the resident hip.Genome from the genome-wide offset offsets[k], reversed where flags[k] & 1 and
    complemented where flags[k] & 2 (3: the minus strand), gathered on the device when the plan is made
    (clh_ends_plan_create_windows); one piece, two pieces and splice alike, DNA matrix only.  Lower-case bases ARE complemented
    here, unlike in Genome.ssw_windows, which keeps the reference's revcomp() quirk (include/ciri_long_hip.h)."""
    _destroy = 'clh_ends_plan_destroy'
    _c, _dtype = 'ends', ENDS_DTYPE

    def __init__(self, ctx, queries, query_off, refs, ref_off, mat, gap_open, gap_extend, mode='global', want_cigar=True, workspace_bytes=0,
                 gap_open2=None, gap_extend2=None, splice=None, strand=None, traceback='stored', windows=None):
        _Handle.__init__(self, ctx)
        if mode not in ENDS_MODES:
            raise ValueError('mode must be one of global, semiglobal, overlap, prefix, extend, got %r' % (mode,))
        if traceback not in ENDS_TRACEBACKS:
            raise ValueError("traceback must be 'stored' or 'recompute', got %r" % (traceback,))
        self.traceback = traceback
        gap2 = gap2_of('EndsPlan', gap_open2, gap_extend2)
        if windows is not None:
            self._create_windows(queries, query_off, refs, ref_off, mat, gap_open, gap_extend, mode, want_cigar, workspace_bytes, gap2, splice, strand, windows)
            return
        if splice is not None:
            self._create_spliced(ctx, queries, query_off, refs, ref_off, mat, gap_open, gap_extend, mode, want_cigar, workspace_bytes, gap2, splice, strand)
            return
        if strand is not None:
            raise ValueError('EndsPlan: strand comes with splice')
        q, q_off, r, r_off, mat, n_mat, _ = self._inputs(queries, query_off, refs, ref_off, mat, want_cigar)
        opts = EndsOpts(ENDS_MODES[mode], mat.ctypes.data, n_mat, int(gap_open), int(gap_extend), ENDS_TRACEBACKS[self.traceback] if self.want_cigar else 0,
                        int(workspace_bytes))
        args = (ctx._h, self.n, q.ctypes.data, q_off.ctypes.data, r.ctypes.data, r_off.ctypes.data, C.byref(opts))
        if gap2 is None:
            self._h = lib().clh_ends_plan_create(*args)
        else:
            self._h = lib().clh_ends_plan_create_gap2(*(args + (C.byref(gap2),)))
        if not self._h:
            raise ClhError('clh_ends_plan_create%s failed: %s' % ('' if gap2 is None else '_gap2', last_error()))

    def _create_windows(self, queries, query_off, refs, ref_off, mat, gap_open, gap_extend, mode, want_cigar, workspace_bytes, gap2, splice, strand, windows):
        """clh_ends_plan_create_windows: one piece, two pieces or introns over windows (genome, offsets, lengths, flags)"""
        if gap2 is not None and splice is not None:
            raise ClhError('clh_ends_plan_create_windows failed: CLH_E_UNSUPPORTED: two-piece gap costs together with introns are not built')
        if strand is not None and splice is None:
            raise ValueError('EndsPlan: strand comes with splice')
        q, q_off, genome, (off, ln, flags), mat, n_mat, _ = self._inputs(queries, query_off, refs, ref_off, mat, want_cigar, windows=windows)
        st = None
        if strand is not None:
            st = np.ascontiguousarray(strand, dtype=np.int8)
            if st.shape != (self.n,):
                raise ValueError('EndsPlan: %d strands for %d pairs' % (st.size, self.n))
        opts = EndsOpts(ENDS_MODES[mode], mat.ctypes.data, n_mat, int(gap_open), int(gap_extend), ENDS_TRACEBACKS[self.traceback] if self.want_cigar else 0,
                        int(workspace_bytes))
        self._h = lib().clh_ends_plan_create_windows(genome._h, self.n, q.ctypes.data, q_off.ctypes.data, off.ctypes.data, ln.ctypes.data, flags.ctypes.data,
                                                     C.byref(opts), C.byref(gap2) if gap2 is not None else None,
                                                     C.byref(splice) if splice is not None else None, st.ctypes.data if st is not None else None)
        if not self._h:
            raise ClhError('clh_ends_plan_create_windows failed: %s' % last_error())

    def _create_spliced(self, ctx, queries, query_off, refs, ref_off, mat, gap_open, gap_extend, mode, want_cigar, workspace_bytes, gap2, splice, strand):
        if gap2 is not None:
            raise ClhError('clh_ends_plan_create_spliced failed: CLH_E_UNSUPPORTED: two-piece gap costs together with introns are not built')
        if not hasattr(lib(), 'clh_ends_plan_create_spliced'):
            raise ClhError('clh_ends_plan_create_spliced: this libclh.so is older than spliced alignment')
        q, q_off, r, r_off, mat, n_mat, _ = self._inputs(queries, query_off, refs, ref_off, mat, want_cigar)
        st = None
        if strand is not None:
            st = np.ascontiguousarray(strand, dtype=np.int8)
            if st.shape != (self.n,):
                raise ValueError('EndsPlan: %d strands for %d pairs' % (st.size, self.n))
        opts = EndsOpts(ENDS_MODES[mode], mat.ctypes.data, n_mat, int(gap_open), int(gap_extend), ENDS_TRACEBACKS[self.traceback] if self.want_cigar else 0,
                        int(workspace_bytes))
        self._h = lib().clh_ends_plan_create_spliced(ctx._h, self.n, q.ctypes.data, q_off.ctypes.data, r.ctypes.data, r_off.ctypes.data, C.byref(opts),
                                                     C.byref(splice), st.ctypes.data if st is not None else None)
        if not self._h:
            raise ClhError('clh_ends_plan_create_spliced failed: %s' % last_error())

    def info(self):
        """the geometry of the kernel: reference columns a lane owns (cpl) and columns of a chunk (a longer reference is walked chunk
        after chunk); and of this plan: shares the batch was cut into so that a share's stored decisions fit the workspace, workspace
        bytes in use, those of the largest pair, pairs the kernels take, pairs with an empty side, CIGAR ops fetch may return; the
        byte counts and the shares are those of the route to the CIGARs in use, `traceback` (None without want_cigar: no route is in use)"""
        out = (C.c_int64 * 8)()
        _check(lib().clh_ends_plan_info(self._h, out), 'clh_ends_plan_info')
        return {'cpl': int(out[0]), 'chunk': int(out[1]), 'shares': int(out[2]), 'workspace_bytes': int(out[3]), 'max_pair_bytes': int(out[4]),
                'kernel_pairs': int(out[5]), 'empty_pairs': int(out[6]), 'cigar_cap': int(out[7]), 'traceback': self.traceback if self.want_cigar else None}


class BandPlan(_PairsPlan):
    """Pairs resident on the GPU for K1gb, the global, semiglobal, prefix and extend programmes of EndsPlan over a band of diagonals
    d = j - i per pair: [min(0, n - m) - band, max(0, n - m) + band] ([-band, band] for 'prefix' and 'extend', whose far end is
    free), or [diagonals[k] - band, diagonals[k] + band] with a hint per pair, clipped
    to [-m, n] and at most 512 wide.  run() any number of times, fetch() (rows BAND_DTYPE, cigars uint32).  A row carries the
    clipped band and `exact`: 1 where it is proved that EndsPlan returns the same row and CIGAR (include/ciri_long_hip.h).
    gap_open2 and gap_extend2 are EndsPlan's two-piece gap costs (clh_band_plan_create_gap2): a byte per cell of the band.
    windows=(genome, offsets, lengths, flags) stands for refs and ref_off as in EndsPlan (clh_band_plan_create_windows)."""
    _destroy = 'clh_band_plan_destroy'
    _c, _dtype = 'band', BAND_DTYPE

    def __init__(self, ctx, queries, query_off, refs, ref_off, mat, gap_open, gap_extend, band, mode='global', diagonals=None, want_cigar=True,
                 workspace_bytes=0, gap_open2=None, gap_extend2=None, windows=None):
        _Handle.__init__(self, ctx)
        if mode not in ENDS_MODES:
            raise ValueError('mode must be one of global, semiglobal, prefix, extend, got %r' % (mode,))
        gap2 = gap2_of('BandPlan', gap_open2, gap_extend2)
        q, q_off, r, r_off, mat, n_mat, diag = self._inputs(queries, query_off, refs, ref_off, mat, want_cigar, diagonals, windows=windows)
        if not 0 <= int(band) < 2 ** 31:
            raise ValueError('BandPlan: band must be a half-width >= 0, got %r' % (band,))
        opts = BandOpts(ENDS_MODES[mode], mat.ctypes.data, n_mat, int(gap_open), int(gap_extend), int(self.want_cigar), int(workspace_bytes), int(band), 0)
        if windows is not None:      # r is the Genome, r_off its windows' offsets, lengths and flags
            self._h = lib().clh_band_plan_create_windows(r._h, self.n, q.ctypes.data, q_off.ctypes.data, r_off[0].ctypes.data, r_off[1].ctypes.data,
                                                         r_off[2].ctypes.data, diag.ctypes.data if diag is not None else None, C.byref(opts),
                                                         C.byref(gap2) if gap2 is not None else None)
            if not self._h:
                raise ClhError('clh_band_plan_create_windows failed: %s' % last_error())
            return
        args = (ctx._h, self.n, q.ctypes.data, q_off.ctypes.data, r.ctypes.data, r_off.ctypes.data, diag.ctypes.data if diag is not None else None,
                C.byref(opts))
        if gap2 is None:
            self._h = lib().clh_band_plan_create(*args)
        else:
            self._h = lib().clh_band_plan_create_gap2(*(args + (C.byref(gap2),)))
        if not self._h:
            raise ClhError('clh_band_plan_create%s failed: %s' % ('' if gap2 is None else '_gap2', last_error()))

    def info(self):
        """the classes of the kernel: band positions a lane owns (cpl; a class holds bands of up to 64 cpl diagonals); and of this plan:
        the greatest clipped width, shares the batch was cut into so that a share's stored decisions fit the workspace, workspace bytes
        in use, those of the largest pair, pairs the kernels take per class, pairs with an empty side, CIGAR ops fetch may return"""
        out = (C.c_int64 * 12)()
        _check(lib().clh_band_plan_info(self._h, out), 'clh_band_plan_info')
        return {'cpl': [int(out[c]) for c in range(3)], 'max_width': int(out[3]), 'shares': int(out[4]), 'workspace_bytes': int(out[5]),
                'max_pair_bytes': int(out[6]), 'class_pairs': [int(out[7 + c]) for c in range(3)], 'empty_pairs': int(out[10]),
                'cigar_cap': int(out[11])}


def flatten_splice_sites(ss_index, offset, length):
    """{contig: {pos: {strand: {'start'|'end': 1}}}} -> (positions int64, counts int64[4]): four strictly ascending runs
    of contig offset + pos in the order '+' starts, '+' ends, '-' starts, '-' ends (clh_genome_set_splice_sites).
    Contigs without an offset, positions outside their contig and strands other than '+'/'-' are left out: no candidate
    can look them up, and a position past the end of a contig must not alias its neighbour."""
    runs = [[], [], [], []]
    for ctg, by_pos in (ss_index or {}).items():
        if ctg not in offset:
            continue
        off, ln = offset[ctg], length[ctg]
        for pos, by_strand in by_pos.items():
            if not 1 <= pos <= ln:
                continue
            for k, strand in enumerate('+-'):
                kinds = by_strand.get(strand) if hasattr(by_strand, 'get') else None
                if not kinds:
                    continue
                if 'start' in kinds:
                    runs[2 * k].append(off + pos)
                if 'end' in kinds:
                    runs[2 * k + 1].append(off + pos)
    runs = [np.unique(np.array(r, dtype=np.int64)) for r in runs]
    cnt = np.array([len(r) for r in runs], dtype=np.int64)
    flat = np.ascontiguousarray(np.concatenate(runs)) if cnt.sum() else np.zeros(1, dtype=np.int64)
    return flat, cnt


class Genome(_Handle):
    """Contigs resident in HBM as base codes (K5).  A Smith-Waterman reference is then a window (contig, start, end,
    minus-strand flag) read in place: no window string, no reverse complement, no per-base encode on the host."""
    _destroy = 'clh_genome_destroy'

    def __init__(self, ctx, contigs):
        """contigs: {name: str} (or an iterable of (name, str)); they are concatenated in iteration order"""
        _Handle.__init__(self, ctx)
        items = list(contigs.items()) if hasattr(contigs, 'items') else list(contigs)
        self.offset, self.length = {}, {}
        pos = 0
        for name, seq in items:
            self.offset[name] = pos; self.length[name] = len(seq); pos += len(seq)
        blob = ''.join(seq for _, seq in items).encode('latin-1')
        self._sites_of = None
        self._h = lib().clh_genome_create(ctx._h, blob, len(blob))
        if not self._h:
            raise ClhError('clh_genome_create failed: %s' % last_error())

    @property
    def codes_ptr(self):
        return lib().clh_genome_codes(self._h)

    def _spans(self, windows):
        off = np.array([self.offset[c] + s for c, s, e in windows], dtype=np.int64)
        ln = np.array([e - s for c, s, e in windows], dtype=np.int64)
        return off, ln

    def count_n(self, windows):
        """upper-case 'N' per window [(contig, start, end)] -- Counter(window)['N'] of find_bsj.py:199"""
        return self.count_n_spans(*self._spans(windows))

    def count_n_spans(self, off, ln):
        """count_n for windows given as genome-wide (offset, length) int64 arrays"""
        off = np.ascontiguousarray(off, dtype=np.int64); ln = np.ascontiguousarray(ln, dtype=np.int64)
        n = len(off)
        out = np.zeros(n, dtype=np.int64)
        if n == 0:
            return out
        _check(lib().clh_genome_count_n(self._h, n, off.ctypes.data, ln.ctypes.data, out.ctypes.data), 'clh_genome_count_n')
        return out

    def letters(self, windows):
        """the letters of windows [(contig, start, end)] as upper-case strings over ACGTN (short spans such as dinucleotides, any number of them: one gather on the device, one lane a span)"""
        if not hasattr(lib(), 'clh_genome_letters'):
            raise ClhError('Genome.letters: this libclh.so is older than the junction refinement')
        off, ln = self._spans(windows)
        out = np.zeros(max(int(ln.sum()), 1), dtype=np.int8)
        _check(lib().clh_genome_letters(self._h, len(off), off.ctypes.data, ln.ctypes.data, out.ctypes.data), 'clh_genome_letters')
        text, at = ''.join('ACGTN'[c] for c in out[:int(ln.sum())]), np.concatenate([[0], np.cumsum(ln)])
        return [text[at[k]:at[k + 1]] for k in range(len(off))]

    def set_splice_sites(self, ss_index):
        """Annotated splice sites for splice_signals(): ss_index = {contig: {pos: {strand: {'start'|'end': 1}}}} (the
        reference's splice_site_index, align.py:235-252) or None.  Contigs that are not resident are ignored."""
        flat, cnt = flatten_splice_sites(ss_index, self.offset, self.length)
        _check(lib().clh_genome_set_splice_sites(self._h, flat.ctypes.data, cnt.ctypes.data), 'clh_genome_set_splice_sites')
        self._sites_of = ss_index

    def splice_signals(self, cands, search_extra=10, shift_threshold=3, is_canonical=True, index_slices=False):
        """K6: cands = [(contig, start, end, clip_base, host_mask)] (or a dict of columns, see below) -> int32 array [n, 8]:
        status, us_free, ds_free, found, strand, us_shift, ds_shift, motif (see include/ciri_long_hip.h).  index_slices: the
        search windows as a minimap2 index serves them (no sequence for a start before the contig) instead of Python slices"""
        if isinstance(cands, dict):       # columns: ctg_off, ctg_len, start, end (int64), clip_base, host_mask (int32)
            off, ln, st, en = (np.ascontiguousarray(cands[k], dtype=np.int64) for k in ('ctg_off', 'ctg_len', 'start', 'end'))
            cb, hm = (np.ascontiguousarray(cands[k], dtype=np.int32) for k in ('clip_base', 'host_mask'))
            n = len(st)
        else:
            n = len(cands)
            off = np.array([self.offset[c[0]] for c in cands], dtype=np.int64)
            ln = np.array([self.length[c[0]] for c in cands], dtype=np.int64)
            st = np.array([c[1] for c in cands], dtype=np.int64)
            en = np.array([c[2] for c in cands], dtype=np.int64)
            cb = np.array([c[3] for c in cands], dtype=np.int32)
            hm = np.array([c[4] for c in cands], dtype=np.int32)
        out = np.zeros((n, 8), dtype=np.int32)
        if n == 0:
            return out
        _check(lib().clh_splice_signal_batch(self._h, n, off.ctypes.data, ln.ctypes.data, st.ctypes.data, en.ctypes.data, cb.ctypes.data,
                                             hm.ctypes.data, search_extra, shift_threshold, (1 if is_canonical else 0) | (2 if index_slices else 0), out.ctypes.data), 'clh_splice_signal_batch')
        return out

    def plan_windows(self, read_off, win_off, win_len, minus, mat, gap_open, gap_extend, flag=1, score_size=2, want_score2=True,
                     want_cigar=True, mask_len=None):
        """A Plan whose references are windows (genome-wide offset, length, minus-strand flag) of this genome:
        plan.run(d_reads_ptr, genome.codes_ptr, stream)."""
        return Plan(self.ctx, read_off, None, mat, gap_open, gap_extend, flag, score_size, want_score2, want_cigar, mask_len,
                    windows=(np.ascontiguousarray(win_off, dtype=np.int64), np.ascontiguousarray(win_len, dtype=np.int32),
                             np.ascontiguousarray(minus, dtype=np.uint8)))

    def ssw_windows(self, reads, read_off, windows, minus, mat, gap_open, gap_extend, flag=1, score_size=2, want_score2=True,
                    want_cigar=True, mask_len=None, spans=None):
        """ssw_batch with reference k = windows[k] = (contig, start, end), reverse-complemented where minus[k].  spans: the windows as
        genome-wide (offset, length) int64 arrays instead (what _spans(windows) gives)."""
        reads = np.ascontiguousarray(reads, dtype=np.int8)
        read_off = np.ascontiguousarray(read_off, dtype=np.int64)
        n = len(read_off) - 1
        off, ln = self._spans(windows) if spans is None else (np.ascontiguousarray(spans[0], dtype=np.int64), np.ascontiguousarray(spans[1], dtype=np.int64))
        ln32 = ln.astype(np.int32)
        rcf = np.ascontiguousarray(np.asarray(minus, dtype=np.uint8))
        o, _keep = self.ctx._opts(mat, gap_open, gap_extend, flag, score_size, want_score2, want_cigar)
        out = np.zeros(n, dtype=ALIGN_DTYPE)
        cap = int(2 * (read_off[-1] if n else 0) + 2 * n + 8) if want_cigar else 1
        cig = np.empty(cap, dtype=np.uint32)     # worst-case capacity; only the used prefix is written
        used = C.c_int64(0)
        ml = np.ascontiguousarray(mask_len, dtype=np.int32) if mask_len is not None else None
        _check(lib().clh_ssw_windows_batch(self._h, n, reads.ctypes.data, read_off.ctypes.data, off.ctypes.data, ln32.ctypes.data, rcf.ctypes.data,
                                           ml.ctypes.data if ml is not None else None, C.byref(o), out.ctypes.data,
                                           cig.ctypes.data if want_cigar else None, cap, C.byref(used)), 'clh_ssw_windows_batch')
        return out, cig[:used.value]


def _packed(reads):
    """reads as libclh takes them: a (codes, offsets) pair as hip.pack gives it, or a list of str / int8 arrays, which is packed"""
    if isinstance(reads, tuple) and len(reads) == 2 and isinstance(reads[1], np.ndarray):
        return np.ascontiguousarray(reads[0], dtype=np.int8), np.ascontiguousarray(reads[1], dtype=np.int64)
    return pack(reads)


class SeedIndex(_Handle):
    """K7: the minimizer index of a resident genome (every contig a sequence of its own), sorted by (key, position) on the device, and
    the two steps that turn reads into loci with it: seeds() and chains().  The definitions -- minimizers with all ties selected,
    anchors, the chain score and the extraction -- are those of include/ciri_long_hip.h; tests/seed_check.py states them in plain
    Python and every array here equals what it gives.  Close the index before its genome."""
    _destroy = 'clh_seed_index_destroy'

    def __init__(self, genome, k=15, w=5, max_occ=64):
        self._h = None
        if not isinstance(genome, Genome) or not genome._h:
            raise ValueError('SeedIndex: genome is an open hip.Genome')
        _Handle.__init__(self, genome.ctx)
        if not hasattr(lib(), 'clh_seed_index_create'):
            raise ClhError('SeedIndex: this libclh.so is older than the minimizer index')
        self.genome, self.k, self.w, self.max_occ = genome, int(k), int(w), int(max_occ)
        self.contigs = list(genome.offset)                  # in the order of the concatenation
        off = np.array([genome.offset[c] for c in self.contigs], dtype=np.int64)
        ln = np.array([genome.length[c] for c in self.contigs], dtype=np.int64)
        self.contig_off = off
        self._h = lib().clh_seed_index_create(genome._h, self.k, self.w, len(off), off.ctypes.data, ln.ctypes.data, self.max_occ)
        if not self._h:
            raise ClhError('clh_seed_index_create failed: %s' % last_error())

    def info(self):
        """entries, distinct keys, keys with more than max_occ entries, device bytes, shares of the last seeds() / chains(), and the
        sketch's geometry: positions a wave decides per round, positions of a work item (one wave), work items of a workgroup"""
        out = (C.c_int64 * 12)()
        _check(lib().clh_seed_index_info(self._h, out), 'clh_seed_index_info')
        return {'entries': int(out[0]), 'distinct': int(out[1]), 'repetitive_keys': int(out[2]), 'bytes': int(out[3]), 'k': int(out[4]), 'w': int(out[5]),
                'max_occ': int(out[6]), 'shares': int(out[7]), 'round': int(out[8]), 'item': int(out[9]), 'items_per_block': int(out[10])}

    def timing(self):
        """HIP-event milliseconds: sketch and sort of the build, the last minimizers() / seeds() on the device, the chain kernels of the last
        chains() / links(), the link kernel of the last links() / link_rows() (the kernel alone, without the
        marker fill of its rows)"""
        ms = (C.c_float * 5)()
        _check(lib().clh_seed_index_timing(self._h, ms), 'clh_seed_index_timing')
        return {'sketch': float(ms[0]), 'sort': float(ms[1]), 'seeds': float(ms[2]), 'chain': float(ms[3]), 'link': float(ms[4])}

    def dump(self, first=0, count=None):
        """entries [first, first + count) of the sorted index -> (keys uint64, genome-wide positions int64, strands uint8)"""
        count = self.info()['entries'] - first if count is None else int(count)
        keys, pos, strand = np.zeros(max(count, 0), dtype=np.uint64), np.zeros(max(count, 0), dtype=np.int64), np.zeros(max(count, 0), dtype=np.uint8)
        _check(lib().clh_seed_index_dump(self._h, int(first), count, keys.ctypes.data, pos.ctypes.data, strand.ctypes.data), 'clh_seed_index_dump')
        return keys, pos, strand

    def minimizers(self, seqs):
        """the index's own sketch on other sequences -> per sequence (positions int64, keys uint64, strands uint8), by position"""
        data, off = _packed(seqs)
        n = len(off) - 1
        moff = np.zeros(n + 1, dtype=np.int64)
        _check(lib().clh_seed_minimizers(self._h, n, data.ctypes.data, off.ctypes.data, moff.ctypes.data), 'clh_seed_minimizers')
        m = int(moff[n])
        pos, keys, strand = np.zeros(m, dtype=np.int64), np.zeros(m, dtype=np.uint64), np.zeros(m, dtype=np.uint8)
        _check(lib().clh_seed_minimizers_fetch(self._h, m, pos.ctypes.data, keys.ctypes.data, strand.ctypes.data), 'clh_seed_minimizers_fetch')
        return [(pos[moff[r]:moff[r + 1]], keys[moff[r]:moff[r + 1]], strand[moff[r]:moff[r + 1]]) for r in range(n)]

    def seeds(self, reads, workspace_bytes=0):
        """the anchors of a batch of reads, in ascending (read, minus, x, y) order -> dict of arrays: anchor_off [n + 1], repetitive [n]
        (minimizers of the read whose key has more than max_occ entries: no anchors), read, minus, x (genome-wide), y"""
        data, off = _packed(reads)
        n = len(off) - 1
        aoff, rep = np.zeros(n + 1, dtype=np.int64), np.zeros(n, dtype=np.int32)
        _check(lib().clh_seed_batch(self._h, n, data.ctypes.data, off.ctypes.data, int(workspace_bytes), aoff.ctypes.data, rep.ctypes.data), 'clh_seed_batch')
        m = int(aoff[n])
        read, minus, x, y = np.zeros(m, dtype=np.int32), np.zeros(m, dtype=np.uint8), np.zeros(m, dtype=np.int64), np.zeros(m, dtype=np.int32)
        _check(lib().clh_seed_batch_fetch(self._h, m, read.ctypes.data, minus.ctypes.data, x.ctypes.data, y.ctypes.data), 'clh_seed_batch_fetch')
        return {'anchor_off': aoff, 'repetitive': rep, 'read': read, 'minus': minus, 'x': x, 'y': y}

    def chains(self, reads, lookback=64, max_gap=5000, max_skew=500, min_score=40, min_anchors=3, max_chains=4, max_attempts=None, workspace_bytes=0):
        """seeds, then colinear chains per (read, strand) on the device -> (chains, truncated): chains[r] the chains of read r, both
        strands merged, ordered by (-score, minus, x_first), each a dict of minus, contig (its index), score, anchors, x_first, y_first,
        x_end, y_end (x inside the contig, y in the read as the strand reads it, ends = start of the last anchor + k); truncated
        [n, 2]: the segment (read, strand) used max_attempts (default 8 max_chains) attempts with a chain end of min_score still unused"""
        data, off = _packed(reads)
        n = len(off) - 1
        o = ChainOpts(int(lookback), int(max_chains), int(8 * max_chains if max_attempts is None else max_attempts), int(min_score), int(min_anchors), 0,
                      int(max_gap), int(max_skew), int(workspace_bytes))
        seg = np.zeros((2 * n, 4), dtype=np.int64)
        rows = np.zeros((2 * n, max(int(max_chains), 1), 10), dtype=np.int64)
        _check(lib().clh_seed_chain_batch(self._h, n, data.ctypes.data, off.ctypes.data, C.byref(o), seg.ctypes.data, rows.ctypes.data), 'clh_seed_chain_batch')
        out = []
        for r in range(n):
            got = [rows[s, c] for s in (2 * r, 2 * r + 1) for c in range(int(seg[s, 0]))]
            got = [{'minus': int(v[1]), 'contig': int(v[2]), 'score': int(v[3]), 'anchors': int(v[4]), 'x_first': int(v[5]), 'y_first': int(v[6]),
                    'x_end': int(v[7]), 'y_end': int(v[8])} for v in got]
            out.append(sorted(got, key=lambda c: (-c['score'], c['minus'], c['x_first'])))
        return out, seg[:, 1].reshape(n, 2).astype(bool)

    @staticmethod
    def _link_opts(max_query_gap, max_overlap, max_skew, max_intron, max_circle, intron_cost, backsplice_cost):
        if not hasattr(lib(), 'clh_seed_link_batch'):
            raise ClhError('SeedIndex: this libclh.so is older than the links between chains')
        return LinkOpts(int(max_query_gap), int(max_overlap), int(max_skew), int(max_intron), int(max_circle), int(intron_cost), int(backsplice_cost))

    def links(self, reads, lookback=64, max_gap=5000, max_skew=500, min_score=40, min_anchors=3, max_chains=32, max_attempts=None, workspace_bytes=0,
              max_query_gap=500, max_overlap=32, max_intron=200000, max_circle=200000, intron_cost=16, backsplice_cost=32):
        """chains() and, behind the chain kernel on the device, the links between the chains of every (read, strand) segment (the
        definitions: include/ciri_long_hip.h, tests/link_check.py; max_skew is the chain's and the link's) -> the raw arrays, segment
        2 r + minus: seg [2 n, 4] (chains, truncated, anchors, 0), rows [2 n, max_chains, 10] (read, minus, contig, score, anchors, x_first,
        y_first, x_end, y_end, 0), link_seg [2 n, 4] (chains, paths, 0, 0), link_rows [2 n, max_chains, 8] (rank, F, pred, kind 0 none /
        1 colinear / 2 intron / 3 back-splice, path, pos, the path's score where pos == 0, 0); only the first `chains` rows of a segment
        are written"""
        data, off = _packed(reads)
        n = len(off) - 1
        lo = self._link_opts(max_query_gap, max_overlap, max_skew, max_intron, max_circle, intron_cost, backsplice_cost)
        o = ChainOpts(int(lookback), int(max_chains), int(8 * max_chains if max_attempts is None else max_attempts), int(min_score), int(min_anchors), 0,
                      int(max_gap), int(max_skew), int(workspace_bytes))
        mc = max(int(max_chains), 1)
        seg, rows = np.zeros((2 * n, 4), dtype=np.int64), np.zeros((2 * n, mc, 10), dtype=np.int64)
        lseg, lrows = np.zeros((2 * n, 4), dtype=np.int64), np.zeros((2 * n, mc, 8), dtype=np.int64)
        _check(lib().clh_seed_link_batch(self._h, n, data.ctypes.data, off.ctypes.data, C.byref(o), C.byref(lo), seg.ctypes.data, rows.ctypes.data,
                                         lseg.ctypes.data, lrows.ctypes.data), 'clh_seed_link_batch')
        return {'seg': seg, 'rows': rows, 'link_seg': lseg, 'link_rows': lrows}

    def link_rows(self, counts, rows, max_query_gap=500, max_overlap=32, max_skew=500, max_intron=200000, max_circle=200000, intron_cost=16,
                  backsplice_cost=32):
        """the links of chain rows the caller gives (another mapper's hits): counts [nseg], rows [nseg, max_chains, 10] in the layout of
        links(), of which contig, score, x_first, y_first, x_end, y_end are read -> link_seg, link_rows as links() gives them"""
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        counts = np.asarray(counts, dtype=np.int64).reshape(-1)
        if rows.ndim != 3 or rows.shape[0] != len(counts) or rows.shape[2] != 10:
            raise ValueError('link_rows: rows is [nseg, max_chains, 10] beside counts [nseg], got %r beside %d' % (rows.shape, len(counts)))
        nseg, mc = int(rows.shape[0]), int(rows.shape[1])
        lo = self._link_opts(max_query_gap, max_overlap, max_skew, max_intron, max_circle, intron_cost, backsplice_cost)
        seg = np.zeros((nseg, 4), dtype=np.int64)
        seg[:, 0] = counts
        lseg, lrows = np.zeros((nseg, 4), dtype=np.int64), np.zeros((nseg, max(mc, 1), 8), dtype=np.int64)
        _check(lib().clh_seed_link_rows(self._h, nseg, mc, seg.ctypes.data, rows.ctypes.data, C.byref(lo), lseg.ctypes.data, lrows.ctypes.data),
               'clh_seed_link_rows')
        return {'link_seg': lseg, 'link_rows': lrows}

    @staticmethod
    def junction_info():
        """K7j's geometry: class_bounds (the greatest m of each class; a class of bound 64 c gives a lane c rows), max_span, max_slack, the
        waves (tasks) of a workgroup"""
        if not hasattr(lib(), 'clh_seed_junction_info'):
            raise ClhError('SeedIndex: this libclh.so is older than the junction refinement')
        out = (C.c_int64 * 8)()
        _check(lib().clh_seed_junction_info(out), 'clh_seed_junction_info')
        return {'class_bounds': [int(v) for v in out[:int(out[7])]], 'max_span': int(out[4]), 'max_slack': int(out[5]), 'waves': int(out[6])}

    def junctions(self, reads, tasks, match=2, mismatch=2, gap_open=3, gap_extend=1, intron_open=12, noncanonical=6, donor_costs=None, acceptor_costs=None,
                  slack=16, max_span=512):
        """back-splice junctions refined to the base (K7j; the definition: include/ciri_long_hip.h, tests/junction_check.py).  tasks [n, 8]:
        read, minus, contig (its index), xd, yd, xa, ya, strand (+1, -1, 0 both) -> [n, 12] int64: status (0 refined, 1 m above max_span,
        2 the anchors cross), score, strand (0 '+', 1 '-'), t, u, v, donor_end, acceptor_start, HL, HR, the start cost, the end cost.  The
        costs are those of ``ssw_wrap.align_windows_spliced``.  last_junction_ms holds the kernels' HIP-event time."""
        if not hasattr(lib(), 'clh_seed_junction_batch'):
            raise ClhError('SeedIndex: this libclh.so is older than the junction refinement')
        data, off = _packed(reads)
        tasks = np.ascontiguousarray(tasks, dtype=np.int64).reshape(-1, 8)
        sp = splice_of('junctions', intron_open, noncanonical, donor_costs, acceptor_costs)
        o = JunctionOpts(int(match), int(mismatch), int(gap_open), int(gap_extend), int(slack), int(max_span))
        out = np.zeros((len(tasks), 12), dtype=np.int64)
        ms = C.c_float(0)
        _check(lib().clh_seed_junction_batch(self._h, len(off) - 1, data.ctypes.data, off.ctypes.data, len(tasks), tasks.ctypes.data, C.byref(o), C.byref(sp),
                                             out.ctypes.data, C.byref(ms)), 'clh_seed_junction_batch')
        self.last_junction_ms = float(ms.value)
        return out

    def circles(self, reads, min_path_score=0, lookback=64, max_gap=5000, max_skew=500, min_score=40, min_anchors=3, max_chains=32, max_attempts=None,
                workspace_bytes=0, max_query_gap=500, max_overlap=32, max_intron=200000, max_circle=200000, intron_cost=16, backsplice_cost=32, match=2,
                mismatch=2, gap_open=3, gap_extend=1, intron_open=12, noncanonical=6, donor_costs=None, acceptor_costs=None, slack=16, max_span=512):
        """the circles of a batch of reads in one device pass (K7c; the definition: include/ciri_long_hip.h, tests/circle_check.py): links()
        and its keywords, the best path of every read with a score of at least min_path_score, junctions() and its keywords on that path's
        back-splice links, the winner's flanks, and the table of the distinct circles; the paths and the tasks stay on the device ->
        dict of arrays: circle [n, 16] int64 (status 0 a circle / 1 no path / 2 no back-splice in the best path / 3 none refined, contig,
        start, end, strand, donor code, acceptor code, J, read_pos, the path's minus, score, chains, back-splice links, those refined, the
        winner's ordinal, 0; a dinucleotide code is 5 c0 + c1, -1 where it leaves the contig), circle_of_read [n] (the read's row of the
        table, -1 without a circle), table [n_circles, 10] (contig, start, end, strand, donor, acceptor, reads, the greatest J, the lowest
        read, 0; ascending), kernel_ms (HIP events: select and task build, the junction kernels, finalise and table)"""
        if not hasattr(lib(), 'clh_seed_circle_batch'):
            raise ClhError('SeedIndex: this libclh.so is older than the circles of a batch')
        data, off = _packed(reads)
        n = len(off) - 1
        lo = self._link_opts(max_query_gap, max_overlap, max_skew, max_intron, max_circle, intron_cost, backsplice_cost)
        o = ChainOpts(int(lookback), int(max_chains), int(8 * max_chains if max_attempts is None else max_attempts), int(min_score), int(min_anchors), 0,
                      int(max_gap), int(max_skew), int(workspace_bytes))
        sp = splice_of('circles', intron_open, noncanonical, donor_costs, acceptor_costs)
        jo = JunctionOpts(int(match), int(mismatch), int(gap_open), int(gap_extend), int(slack), int(max_span))
        circle, of_read = np.zeros((n, 16), dtype=np.int64), np.zeros(n, dtype=np.int64)
        count = C.c_int64(0)
        ms = (C.c_float * 3)()
        _check(lib().clh_seed_circle_batch(self._h, n, data.ctypes.data, off.ctypes.data, C.byref(o), C.byref(lo), C.byref(jo), C.byref(sp), int(min_path_score),
                                           circle.ctypes.data, of_read.ctypes.data, C.byref(count), ms), 'clh_seed_circle_batch')
        table = np.zeros((int(count.value), 10), dtype=np.int64)
        _check(lib().clh_seed_circle_table_fetch(self._h, int(count.value), table.ctypes.data), 'clh_seed_circle_table_fetch')
        return {'circle': circle, 'circle_of_read': of_read, 'table': table, 'kernel_ms': np.array([float(v) for v in ms], dtype=np.float32)}


class Plan(_Handle):
    """A batch shape resident on the GPU: run() it on device pointers any number of times."""
    _destroy = 'clh_plan_destroy'

    def __init__(self, ctx, read_off, ref_off, mat, gap_open, gap_extend, flag, score_size, want_score2, want_cigar, mask_len,
                 windows=None):
        _Handle.__init__(self, ctx)
        L = lib()
        self.read_off = np.ascontiguousarray(read_off, dtype=np.int64)
        self.n = len(self.read_off) - 1
        self.want_cigar = bool(want_cigar)
        o, self._mat = ctx._opts(mat, gap_open, gap_extend, flag, score_size, want_score2, want_cigar)
        ml = np.ascontiguousarray(mask_len, dtype=np.int32) if mask_len is not None else None
        if windows is not None:
            self._win = windows
            self._h = L.clh_ssw_plan_windows(ctx._h, self.n, self.read_off.ctypes.data, windows[0].ctypes.data, windows[1].ctypes.data,
                                             windows[2].ctypes.data, ml.ctypes.data if ml is not None else None, C.byref(o))
        else:
            self.ref_off = np.ascontiguousarray(ref_off, dtype=np.int64)
            self._h = L.clh_ssw_plan(ctx._h, self.n, self.read_off.ctypes.data, self.ref_off.ctypes.data,
                                     ml.ctypes.data if ml is not None else None, C.byref(o))
        if not self._h:
            raise ClhError('clh_ssw_plan failed: %s' % last_error())

    def run(self, d_reads_ptr, d_refs_ptr, stream=0):
        """stream: a hipStream_t handle (e.g. torch.cuda.Stream().cuda_stream).  0 selects libclh's own private stream, which
        is NOT ordered with torch's default stream: pass the stream your inputs are produced on.  With a matrix of edge 6..32 and
        CIGARs wanted, the two buffers must stay allocated and unmodified until fetch() returns: fetch() may run tracebacks again
        on libclh's own stream, and they read them (include/ciri_long_hip.h: clh_ssw_fetch)."""
        _check(lib().clh_ssw_run(self._h, C.c_void_p(d_reads_ptr), C.c_void_p(d_refs_ptr), C.c_void_p(stream)), 'clh_ssw_run')

    def fetch(self):
        out = np.zeros(self.n, dtype=ALIGN_DTYPE)
        cap = int(2 * (self.read_off[-1] if self.n else 0) + 2 * self.n + 8) if self.want_cigar else 1
        cig = np.empty(cap, dtype=np.uint32)     # worst-case capacity; only the used prefix is ever written or touched
        used = C.c_int64(0)
        _check(lib().clh_ssw_fetch(self._h, out.ctypes.data, cig.ctypes.data if self.want_cigar else None, cap, C.byref(used)), 'clh_ssw_fetch')
        return out, cig[:used.value]

    def set_refs_bytes(self, nbytes):
        """state the size of the refs buffer handed to run() (include/ciri_long_hip.h: padding contract of d_refs); -1 = unstated"""
        lib().clh_plan_set_refs_bytes(self._h, int(nbytes))

    def set_profiling(self, on=True):
        lib().clh_plan_set_profiling(self._h, 1 if on else 0)

    def segments(self):
        """[(rows-per-lane class, alignments, read bases, ref bases)] in launch order"""
        rv = np.zeros(32, dtype=np.int32); cnt = np.zeros(32, dtype=np.int32)
        rb = np.zeros(32, dtype=np.int64); fb = np.zeros(32, dtype=np.int64)
        ns = lib().clh_plan_segments(self._h, 32, rv.ctypes.data, cnt.ctypes.data, rb.ctypes.data, fb.ctypes.data)
        return [(int(rv[k]), int(cnt[k]), int(rb[k]), int(fb[k])) for k in range(ns)]

    def traceback_counts(self):
        """(alignments handed to the wide row traceback, alignments handed on to the anti-diagonal traceback) of the last run"""
        c = np.zeros(2, dtype=np.int32)
        _check(lib().clh_plan_traceback_counts(self._h, c.ctypes.data), 'clh_plan_traceback_counts')
        return int(c[0]), int(c[1])

    def prefilter_stats(self):
        """what the exact column prefilter (csrc/ssw_prefilter.hip) did in the last run: alignments of the sliced scan class, of
        them with candidate slices, slices run, window columns computed, window columns of the class, alignments that also went
        through the second stage (indel-distance bound)"""
        c = np.zeros(6, dtype=np.int64)
        _check(lib().clh_plan_prefilter_stats(self._h, c.ctypes.data), 'clh_plan_prefilter_stats')
        return dict(zip(('alignments', 'pruned', 'slices', 'cols_computed', 'cols_window', 'second_stage'), (int(x) for x in c)))

    def prefilter_timing(self):
        """ssw_prefilter_kernel alone in the last profiling run, per long-window class (reads up to 254 bases, longer reads):
        [(ms, window columns x W words, the same x (11 W + 8) instructions per column and lane), ...]"""
        ms = np.zeros(2, dtype=np.float32); w = np.zeros(4, dtype=np.int64)
        _check(lib().clh_plan_prefilter_timing(self._h, ms.ctypes.data, w.ctypes.data), 'clh_plan_prefilter_timing')
        return [(float(ms[k]), int(w[2 * k]), int(w[2 * k + 1])) for k in range(2)]

    def timing(self):
        """([K1 ms per segment], (K1b small-window ms, K1b large-window ms)) for the last run"""
        a = np.zeros(32, dtype=np.float32); b = np.zeros(2, dtype=np.float32)
        ns = lib().clh_plan_timing(self._h, 32, a.ctypes.data, b.ctypes.data)
        if ns < 0:
            _check(ns, 'clh_plan_timing')
        return [float(a[k]) for k in range(ns)], (float(b[0]), float(b[1]))

    def results_dev_ptr(self):
        return lib().clh_ssw_results_dev(self._h)


class CcsPlan(_Handle):
    """Consensus step for a batch shape resident on the GPU (K2 + K3)."""
    _destroy = 'clh_ccs_plan_destroy'

    def __init__(self, ctx, read_off):
        _Handle.__init__(self, ctx)
        self.read_off = np.ascontiguousarray(read_off, dtype=np.int64)
        self.n = len(self.read_off) - 1
        self._h = lib().clh_ccs_plan_create(ctx._h, self.n, self.read_off.ctypes.data)
        if not self._h:
            raise ClhError('clh_ccs_plan_create failed: %s' % last_error())

    def run(self, d_reads_ptr, stream=0):
        """stream: see Plan.run"""
        _check(lib().clh_ccs_run(self._h, C.c_void_p(d_reads_ptr), C.c_void_p(stream)), 'clh_ccs_run')

    def timing(self):
        """(K2 ms, K3 ms) of the last run"""
        ms = np.zeros(2, dtype=np.float32)
        _check(lib().clh_ccs_plan_timing(self._h, ms.ctypes.data), 'clh_ccs_plan_timing')
        return float(ms[0]), float(ms[1])

    def info(self):
        """dict(slots, slot_bytes, big_slots, big_slot_bytes, ran_in_claimed_big_slot, ran_in_second_launch) of the last run"""
        out = np.zeros(6, dtype=np.int64)
        _check(lib().clh_ccs_plan_info(self._h, out.ctypes.data), 'clh_ccs_plan_info')
        return dict(zip(('slots', 'slot_bytes', 'big_slots', 'big_slot_bytes', 'ran_in_claimed_big_slot', 'ran_in_second_launch'), (int(x) for x in out)))

    def stats(self):
        """dict(dp_cells, dp_row_steps, dropped = {status: reads}) of the last run; `dropped` lists the reads a limit of the kernel left
        without a consensus (status 1 workspace, 2 graph limits, 3 output, 4 (unused since round 4), 5 back-track guard, 6 16-bit
        range, 7 alignment without a base)"""
        out = np.zeros(16, dtype=np.int64)
        _check(lib().clh_ccs_plan_stats(self._h, out.ctypes.data), 'clh_ccs_plan_stats')
        return {'dp_cells': int(out[0]), 'dp_row_steps': int(out[1]), 'band_misses': int(out[2]), 'dropped': {k: int(out[2 + k]) for k in range(1, 8) if out[2 + k]}}

    def results_dev(self):
        """device pointers (rows, segs, ccs) of the last run's outputs; ccs is packed at the read offsets"""
        a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(lib().clh_ccs_results_dev(self._h, C.byref(a), C.byref(b), C.byref(c)), 'clh_ccs_results_dev')
        return a.value, b.value, c.value

    def fetch(self):
        out = np.zeros(self.n, dtype=CCS_DTYPE)
        segs = np.zeros((self.n, CCS_SEG_CAP, 2), dtype=np.int32)
        ccs = np.zeros(max(1, int(self.read_off[-1])), dtype=np.int8)
        _check(lib().clh_ccs_fetch(self._h, out.ctypes.data, segs.ctypes.data, ccs.ctypes.data), 'clh_ccs_fetch')
        return out, segs, ccs


_default_ctx = {}


def default_context(device=None):
    if device is None:
        device = int(os.environ.get('CIRI_LONG_DEVICE', os.environ.get('LOCAL_RANK', '0')))
    if device not in _default_ctx:
        _default_ctx[device] = Context(device)
    return _default_ctx[device]
