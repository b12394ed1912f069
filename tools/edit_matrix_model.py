"""csrc/edit_matrix.hip in Python: the two pieces of index arithmetic the kernels rest on.

  pair_of(q, n)     position q of the condensed upper triangle of n items -> (i, j), i < j, in np.triu_indices(n, 1) order;
                    em_pair_of of the kernel: a floating square root proposes the row, two integer loops make it exact.
  keep_mask(s)      which bytes homopolymer compression keeps: byte i iff i == 0 or s[i] != s[i-1];
  compress_waves(s) hpc_compress_kernel's walk over a string: steps of 64 bytes, the write position of a kept byte is the
                    running length plus the kept bytes in lower lanes of its step.

tests/test_edit_matrix_host.py holds them against np.triu_indices and utils.compress_seq."""
import math


def pair_of(q, n):
    r = n * (n - 1) // 2 - 1 - q                      # pairs behind q
    k = int((math.sqrt(float(8 * r + 1)) - 1.0) * 0.5)
    while k > 0 and k * (k + 1) // 2 > r:
        k -= 1
    while (k + 1) * (k + 2) // 2 <= r:
        k += 1
    i = n - 2 - k                                     # row i holds q iff k (k + 1) / 2 <= r < (k + 1) (k + 2) / 2
    return i, q - i * (2 * n - i - 1) // 2 + i + 1


def row_start(i, n):
    """position of pair (i, i + 1)"""
    return i * (2 * n - i - 1) // 2


def keep_mask(s):
    return [i == 0 or s[i] != s[i - 1] for i in range(len(s))]


def compress_waves(s):
    out = [None] * len(s)
    kept = 0
    for base in range(0, len(s), 64):
        keep = [base + lane < len(s) and (base + lane == 0 or s[base + lane] != s[base + lane - 1]) for lane in range(64)]
        for lane in range(64):
            if keep[lane]:
                out[kept + sum(keep[:lane])] = s[base + lane]
        kept += sum(keep)
    return out[:kept]


def lane_group(pat_len):
    """ed_group of clh_api.hip: lanes a pair occupies in K4"""
    blocks, g = (pat_len + 63) >> 6, 1
    while g < blocks and g < 64:
        g <<= 1
    return g
