"""K6 (splice_scan_kernel of csrc/splice_scan.hip) stated in Python, step for step as the kernel computes it and not as
oracle/splice_oracle.c states the result: the byte layout of the resident genome (K5: code, lower-case bit, N bit), the flank
comparison on characters, the two slices as (first index, length), the annotated sites as 64-bit masks over the shifts [-sl, sl)
taken by binary search in four genome-wide runs, the packed ranking key with its 15-bit fields and a running strict minimum, and the
de-novo double loop over lo / lo0 / hi_u / hi_d with the annotated shifts joining the motif occurrences.

The motif tables, the key's field order and shifts, the slide cap and the mask width are parsed out of splice_scan.hip
(`constants()`); a form that cannot be parsed raises.

`fault=` plants one wrong rule in THIS text (tests/test_splice_edges_host.py shows each caught by a named set of tests/splice_edges.py):
 1 `key <= best`                     2 mask origin one further: shift -sl lost, shift sl gained
 3 start kind looked up at pos       4 edge rule `<= 0`                 5 free-slide cap one higher
 6 motif search from index 0         7 tier 0 as `alt < cb`             8 tier-1 key with w before alt
 9 minus-strand motifs keep sides   10 negative start clamped to 0     11 short_seq with `<=`
12 flanks compared on codes         13 second round skipped"""
import bisect
import os
import re

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'ciri_long_amd', 'csrc')
SOURCE = os.path.join(_CSRC, 'splice_scan.hip')
FAULTS = tuple(range(1, 14))
U64 = (1 << 64) - 1


def constants(source=SOURCE):
    """kDonor, kAcceptor, kWeight; KEY = per tier class (0, 1, 2) the fields (name, shift) from high to low; TIER_SHIFT; SLIDE_CAP;
    MASK_BITS.  ValueError where a form is not found."""
    with open(source) as f:
        src = f.read()
    K = {}
    for name in ('kDonor', 'kAcceptor'):
        m = re.search(r'uint8_t %s\[5\]\[2\] = \{((?:\{\d, \d\}(?:, )?){5})\};' % name, src)
        if not m:
            raise ValueError('splice_scan_model: %s not found in %s' % (name, source))
        K[name] = [tuple(int(x) for x in p) for p in re.findall(r'\{(\d), (\d)\}', m.group(1))]
    m = re.search(r'uint8_t kWeight\[5\] = \{(\d), (\d), (\d), (\d), (\d)\};', src)
    if not m:
        raise ValueError('splice_scan_model: kWeight not found in %s' % source)
    K['kWeight'] = [int(x) for x in m.groups()]
    body = src[src.index('unsigned long long site_key('):src.index('template <bool ANNO>')]
    keys = re.findall(r'key = \((\w+) << (\d+)\)((?: \| \(\(unsigned long long\)\w+ << \d+\)){3});', body)
    if len(keys) != 3 or [k[0] for k in keys] != ['0ull', '1ull', 'tier'] or 'return key | (unsigned long long)tot;' not in body:
        raise ValueError('splice_scan_model: site_key() in %s no longer has the form this parser reads' % source)
    K['TIER_SHIFT'] = int(keys[0][1])
    K['KEY'] = [[(n, int(s)) for n, s in re.findall(r'\(unsigned long long\)(\w+) << (\d+)', k[2])] for k in keys]
    for fields in K['KEY']:
        sh = [s for _, s in fields]
        if sh != sorted(sh, reverse=True) or len({a - b for a, b in zip(sh, sh[1:] + [0])}) != 1:
            raise ValueError('splice_scan_model: the key fields of %s are not equally wide' % source)
    K['FIELD_BITS'] = K['KEY'][0][-1][1]
    caps = re.findall(r'for \(int [ij] = 1; [ij] < (\d+); \+\+[ij]\)', src)
    m = re.search(r'use_anno && 2 \* sl > (\d+)\)', src)
    if len(caps) != 2 or caps[0] != caps[1] or not m:
        raise ValueError('splice_scan_model: the slide loops or the mask rule of %s no longer have the form this parser reads' % source)
    K['SLIDE_CAP'] = int(caps[0])
    K['MASK_BITS'] = int(m.group(1))
    return K


def encode(text):
    """K5's byte per character (genome.hip: encode_base): bits 0-2 code, bit 3 lower-case acgt, bit 4 upper-case N"""
    raw = text if isinstance(text, bytes) else text.encode('latin-1')
    out = bytearray(len(raw))
    for k, ch in enumerate(raw):
        code = {65: 0, 67: 1, 71: 2, 84: 3}.get(ch & 0xdf, 4)
        if not 97 <= (ch | 0x20) <= 122:
            code = 4
        out[k] = code | (8 if code < 4 and ch & 0x20 else 0) | (16 if ch == 78 else 0)
    return bytes(out)


def site_mask(a, g0, span):
    m = 0
    for k in range(bisect.bisect_left(a, g0), len(a)):
        d = a[k] - g0
        if d >= span:
            break
        m |= 1 << d
    return m & U64


def _bits(m):
    while m:
        low = m & -m
        yield low.bit_length() - 1
        m ^= low


def site_key(i, j, w, cb, us_free, ds_free, K, fault=0):
    v = {'w': w, 'alt': abs(i - j), 'clip_alt': min(abs(j - i - cb), abs(j - i + cb))}
    tot = min(abs(i + us_free), abs(i - ds_free)) + min(abs(j + us_free), abs(j - ds_free))
    if (v['alt'] < cb) if fault == 7 else (v['alt'] <= cb):
        tier, fields = 0, K['KEY'][0]
    elif -us_free <= i <= ds_free and -us_free <= j <= ds_free:
        tier, fields = 1, K['KEY'][1]
        if fault == 8:
            fields = [(K['KEY'][2][k][0], fields[k][1]) for k in range(3)]
    else:
        tier, fields = (2 if -cb <= i <= 0 <= j <= cb else 3), K['KEY'][2]
    key = tier << K['TIER_SHIFT']
    for name, shift in fields:
        key |= v[name] << shift
    return (key | tot) & U64


def scan(codes, ascii_, task, search_extra, shift_threshold, flags, sites, K=None, fault=0):
    """One lane.  codes / ascii_: the whole genome as K5 holds it (encode(text), text as bytes); task = (ctg_off, ctg_len, start, end,
    clip_base, host_mask); sites = four ascending lists of genome-wide positions, or None where none are loaded (the kernel without
    them) -> the row of eight."""
    K = K or constants()
    off, L, S, E, cb, host_mask = task
    anno = bool(sites) and sum(len(r) for r in sites) > 0
    index_slices, canonical = bool(flags & 2), flags & 1
    status = 1 if (S < 0 or S >= E or E > L) else 0
    us_free = ds_free = 0
    cap = K['SLIDE_CAP'] + (1 if fault == 5 else 0)

    def same(a, b):
        if fault == 12:
            return codes[off + a] & 7 == codes[off + b] & 7
        return ascii_[off + a] == ascii_[off + b]
    if not status:
        for i in range(1, cap):
            if E + i > L or not same(S + i - 1, E + i - 1):
                break
            ds_free = i
        for j in range(1, cap):
            if S - j < 0 or not same(S - j, E - j):
                break
            us_free = j
    sl = cb + search_extra
    us_len, ds_len = sl + us_free, sl + ds_free
    edge = (S - us_len - 2 <= 0 if fault == 4 else S - us_len - 2 < 0) or E + ds_len + 2 > L

    def pyslice(a, b):
        if index_slices:
            if a < 0 or a >= L or a >= b:
                return 0, -1
            return a, min(b, L) - a
        if a < 0:
            a = 0 if fault == 10 else max(a + L, 0)
        elif a > L:
            a = L
        if b < 0:
            b = max(b + L, 0)
        elif b > L:
            b = L
        return a, max(b - a, 0)
    ua, nu = pyslice(S - us_len - 2, S + ds_len)
    da, nd = pyslice(E - us_len, E + ds_len + 2)
    need = ds_len - us_len + 2
    short_seq = nu < 0 or nd < 0 or ((nu <= need or nd <= need) if fault == 11 else (nu < need or nd < need))
    pu, pd = off + ua + us_len, off + da + us_len
    row = [0, us_free, ds_free, 0, 0, 0, 0, 0]
    use_anno = anno and not edge
    row[0] = 1 if (not status and use_anno and 2 * sl > K['MASK_BITS']) else status
    if row[0]:
        return row
    T = cb + shift_threshold
    best, found, win = U64, 0, (0, 0, 0, 0)
    mu = [[0, 0], [0, 0]]
    md = [[0, 0], [0, 0]]
    org = 1 if fault == 2 else 0           # the masks' origin: bit k is shift k - sl + org

    def better(key):
        return key <= best if fault == 1 else key < best
    if use_anno:
        gs, ge = off + S - sl + org, off + E - sl + org
        st = 0 if fault == 3 else 1
        for s in range(2):
            mu[s] = [site_mask(sites[2 * s], gs + st, 2 * sl), site_mask(sites[2 * s + 1], gs, 2 * sl)]
            md[s] = [site_mask(sites[2 * s], ge + st, 2 * sl), site_mask(sites[2 * s + 1], ge, 2 * sl)]
        g = codes
        for s in range(2):
            for pi in range(2):
                for bi in _bits(mu[s][pi]):
                    i = bi - sl + org
                    u0, u1 = g[off + S + i - 2], g[off + S + i - 1]
                    for pj in range(2):
                        for bj in _bits(md[s][pj]):
                            j = bj - sl + org
                            if abs(i - j) > T:
                                continue
                            d0, d1 = g[off + E + j], g[off + E + j + 1]
                            w = 3
                            if u0 < 4 and u1 < 4 and d0 < 4 and d1 < 4:
                                n0, n1 = (3 - u1, 3 - u0) if s else (d0, d1)
                                a0, a1 = (3 - d1, 3 - d0) if s else (u0, u1)
                                for m in range(5):
                                    if K['kDonor'][m] == (n0, n1) and K['kAcceptor'][m] == (a0, a1):
                                        w = K['kWeight'][m]
                            key = site_key(i, j, w, cb, us_free, ds_free, K, fault)
                            if better(key):
                                best, found, win = key, 2, (s, i, j, 0)
    lo = (0 if fault == 6 else 1) - us_len
    hi_u, hi_d = nu - 2 - us_len, nd - 2 - us_len
    alo, ahi = -sl + org, sl - 1 + org
    lo0 = min(lo, alo) if use_anno else lo
    host = host_mask & 3
    g = codes
    for rnd in range(2):
        if found or short_seq or (rnd == 1 and (host == 0 or fault == 13)):
            break
        mask = (host if host else 3) if rnd == 0 else (3 & ~host)
        for s in range(2):
            if not (mask >> s) & 1:
                continue
            au, ad = mu[s][0] | mu[s][1], md[s][0] | md[s][1]
            for m in range(1 if canonical else 5):
                D, A = K['kDonor'][m], K['kAcceptor'][m]
                if s == 0:
                    u0, u1, d0, d1 = A[0], A[1], D[0], D[1]
                elif fault == 9:
                    u0, u1, d0, d1 = 3 - A[1], 3 - A[0], 3 - D[1], 3 - D[0]
                else:
                    u0, u1, d0, d1 = 3 - D[1], 3 - D[0], 3 - A[1], 3 - A[0]
                w = K['kWeight'][m]
                hi_i = max(hi_u, ahi) if use_anno else hi_u
                hi_j = max(hi_d, ahi) if use_anno else hi_d
                js = None
                for i in range(lo0, hi_i + 1):
                    ai = use_anno and alo <= i <= ahi and (au >> (i + sl - org)) & 1
                    if not ai and (i < lo or i > hi_u or g[pu + i] != u0 or g[pu + i + 1] != u1):
                        continue
                    if js is None:         # the downstream sites of this strand and motif, found once (the kernel rereads them per i)
                        js = [j for j in range(lo0, hi_j + 1)
                              if (use_anno and alo <= j <= ahi and (ad >> (j + sl - org)) & 1) or
                              not (j < lo or j > hi_d or g[pd + j] != d0 or g[pd + j + 1] != d1)]
                    for j in js:
                        if j < max(lo0, i - T) or j > min(hi_j, i + T):
                            continue
                        key = site_key(i, j, w, cb, us_free, ds_free, K, fault)
                        if better(key):
                            best, found, win = key, 1, (s, i, j, m)
    row[3] = found
    row[4:8] = win
    return row


class Genome(object):
    """contigs = [(name, text)] in genome order, as K5 holds them; row() is scan() for cand = (name, start, end, clip_base, host_mask)"""

    def __init__(self, contigs):
        self.text = ''.join(t for _, t in contigs).encode('latin-1')
        self.codes = encode(self.text)
        self.span, at = {}, 0
        for name, t in contigs:
            self.span[name] = (at, len(t)); at += len(t)

    def row(self, cand, search_extra=10, shift_threshold=3, flags=0, sites=None, K=None, fault=0):
        off, L = self.span[cand[0]]
        return scan(self.codes, self.text, (off, L, cand[1], cand[2], cand[3], cand[4]), search_extra, shift_threshold, flags, sites, K, fault)
