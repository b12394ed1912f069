"""K2 (ccs_scan_kernel, ccs_scan_kernel_x4, ccs_scan_long_kernel of csrc/ccs_poa.hip) stated in Python, step for step as the kernel
computes it and not as oracle/ccs_oracle.c states the result: k-mer codes and their validity, the hash buckets and their chains, every
pair of equal codes visited once from next[i], the clipped smoothing, per-thread strided maxima merged by the kernel's comparisons
(butterfly inside a wave, then the waves in order), the harmonic loop, and per cut the window walk from the bucket heads, the vote
histogram, the strided vote merge and the guarded anchor search with its `dist > ad` skip and four-key `closer`.

The model is parameterised by what must NOT change the answer: NT (threads on a read; 64 and 256 in the kernels), nbuckets (512, 1024,
2048 in the kernels) and the order in which the positions enter their chains (atomicExch: any order on the device).
tests/test_ccs_edges_host.py holds it to clo_ccs_segments over a grid of the three and plants one-line faults in this text.

Constants are parsed out of the sources (`constants()`); a form that cannot be parsed raises."""
import os
import re

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'ciri_long_amd', 'csrc')
SOURCE = os.path.join(_CSRC, 'ccs_poa.hip')
API = os.path.join(_CSRC, 'clh_api.hip')
DEVICE_H = os.path.join(_CSRC, 'clh_device.h')

_INTS = ('CCS_K', 'CCS_DMIN', 'CCS_MIN_SUPPORT', 'CCS_SMOOTH', 'CCS_MAX_CUTS', 'CCS_MIN_TAIL', 'CCS_GUARD', 'K2_BUCKETS', 'K2_WIDE_FROM',
         'K2_LDS_MAX')
INT_MAX = 0x7fffffff


def constants(source=SOURCE, api=API, device_h=DEVICE_H):
    """CCS_*, K2_* and the steps of k2_buckets from ccs_poa.hip, the class ladder T[] from clh_api.hip, kK2LdsMax and CCS_SEG_CAP from
    clh_device.h.  KeyError / ValueError where a name or a form is not found."""
    with open(source) as f:
        src = f.read()
    with open(api) as f:
        api_src = f.read()
    with open(device_h) as f:
        dev = f.read()
    K = {}
    for name in _INTS:
        m = re.search(r'^static constexpr int %s = (\d+);' % name, src, re.M)
        if not m:
            raise KeyError('ccs_scan_model: %s not found in %s' % (name, source))
        K[name] = int(m.group(1))
    m = re.search(r'inline int k2_buckets\(int lcap\) \{ return lcap <= (\d+) \? (\d+) : \(lcap <= (\d+) \? (\d+) : (\d+)\); \}', src)
    if not m:
        raise ValueError('ccs_scan_model: k2_buckets() in %s no longer has the form this parser reads' % source)
    a, na, b, nb, top = (int(x) for x in m.groups())
    K['BUCKET_STEPS'] = ((a, na), (b, nb))
    K['BUCKETS_TOP'] = top
    m = re.search(r'static const int T\[\] = \{([\d, ]+)\};', api_src)
    if not m or 'pl->lcap = (std::min(lmax, clh::kK2LdsMax) + 63) & ~63;' not in api_src:
        raise ValueError('ccs_scan_model: the K2 launch classes in %s no longer have the form this parser reads' % api)
    K['T'] = tuple(int(x) for x in m.group(1).split(','))
    for name in ('kK2LdsMax', 'CCS_SEG_CAP'):
        m = re.search(r'static constexpr int %s = (\d+);' % name, dev)
        if not m:
            raise KeyError('ccs_scan_model: %s not found in %s' % (name, device_h))
        K[name] = int(m.group(1))
    if K['kK2LdsMax'] != K['K2_LDS_MAX'] or K['BUCKETS_TOP'] != K['K2_BUCKETS'] or K['CCS_SEG_CAP'] != K['CCS_MAX_CUTS'] + 1:
        raise ValueError('ccs_scan_model: the sources disagree about K2_LDS_MAX, K2_BUCKETS or CCS_SEG_CAP')
    return K


def k2_buckets(lcap, K):
    for limit, n in K['BUCKET_STEPS']:
        if lcap <= limit:
            return n
    return K['BUCKETS_TOP']


def batch_lcap(lengths, K):
    """the plan's lcap: the batch's longest read, at most kK2LdsMax, rounded up to 64"""
    return (min(max(list(lengths) + [1]), K['kK2LdsMax']) + 63) & ~63


def class_of(L, lcap, K):
    """the launch class (its lcap) of a read of L bases in a batch of that lcap; reads above kK2LdsMax are filed under kK2LdsMax"""
    L = min(L, K['kK2LdsMax'])
    for t in K['T']:
        if L <= t:
            return min(t, lcap)
    return lcap


def route(L, lengths, K, one_wave=False):
    """(kernel, buckets) that scans a read of L bases in a batch of `lengths`"""
    if L > K['kK2LdsMax']:
        return 'long', K['K2_BUCKETS']
    c = class_of(L, batch_lcap(lengths, K), K)
    return ('x4' if c >= K['K2_WIDE_FROM'] and not one_wave else 'one wave'), k2_buckets(c, K)


def _butterfly(lanes, better):
    """__shfl_xor over 1, 2, .. 32 in every wave of 64: a lane takes the other's answer where `better` says so; -> lane 0 of every wave"""
    lanes = list(lanes)
    for d in (1, 2, 4, 8, 16, 32):
        lanes = [lanes[k ^ d] if better(lanes[k ^ d], lanes[k]) else lanes[k] for k in range(len(lanes))]
    return lanes[::64]


def _merge(lanes, empty, better):
    """the answers of NT threads: butterfly in each wave (threads a wave does not have hold `empty`), then the waves in order"""
    lanes = list(lanes) + [empty] * (-len(lanes) % 64)
    waves = _butterfly(lanes, better)
    out = waves[0]
    for w in waves[1:]:
        if better(w, out):
            out = w
    return out


def scan(seq, NT=64, nbuckets=None, order='ascending', K=None, stats=None):
    """ccs_scan_read on one read of int codes -> (period, ncuts, support, cuts); (0, 0, 0, []) without a repeat.
    order: 'ascending' | 'descending' | a list of positions: the order in which atomicExch puts the positions into their chains.
    stats: a dict that receives 'longest_chain' and 'unequal_visits' (chain steps of the period count onto another code)."""
    K = K or constants()
    k, DMIN, SMOOTH, GUARD = K['CCS_K'], K['CCS_DMIN'], K['CCS_SMOOTH'], K['CCS_GUARD']
    seq = [int(x) for x in seq]
    L = len(seq)
    none = (0, 0, 0, [])
    if L < 2 * DMIN:
        return none
    if nbuckets is None:
        nbuckets = k2_buckets((min(L, K['kK2LdsMax']) + 63) & ~63, K) if L <= K['kK2LdsMax'] else K['K2_BUCKETS']
    dmax = L // 2
    # codes; a k-mer is valid if it lies in the read and holds only 0..3
    code, next_ = [0] * L, [-2] * L
    head = [-1] * nbuckets
    valid = [False] * L
    for i in range(L):
        ok = i + k <= L
        c = 0
        if ok:
            for t in range(k):
                b = seq[i + t]
                if b < 0 or b > 3:
                    ok = False
                c = (c << 2) | (b & 3)
        code[i] = c & 0xffff
        valid[i] = ok
    positions = range(L) if order == 'ascending' else (range(L - 1, -1, -1) if order == 'descending' else order)
    for i in positions:
        if valid[i]:
            c = code[i]
            h = (c ^ (c >> 5)) & (nbuckets - 1)
            next_[i], head[h] = head[h], i
    # one count per pair of equal codes: from next[i] on, the positions of the bucket that entered before i
    cnt = {d: 0 for d in range(DMIN, dmax + 1)}             # cnt exists over [DMIN, L/2] alone
    longest = unequal = 0
    for i in range(L):
        j = next_[i]
        if j == -2:
            continue
        ci = code[i]
        steps = 0
        while j >= 0:
            steps += 1
            if code[j] == ci:
                d = i - j if i > j else j - i
                if d >= DMIN and d <= dmax:
                    cnt[d] += 1
            else:
                unequal += 1
            j = next_[j]
        longest = max(longest, steps + 1)
    if stats is not None:
        stats['longest_chain'], stats['unequal_visits'] = longest, unequal
    # smoothed counts; a thread's offsets ascend, so its `>` keeps the smallest of its maxima
    sm = {}
    lanes = []
    for lane in range(NT):
        best, bestd = -1, INT_MAX
        for d in range(DMIN + lane, dmax + 1, NT):
            lo = max(d - SMOOTH, DMIN)
            hi = min(d + SMOOTH, dmax)
            s = sum(cnt[e] for e in range(lo, hi + 1))
            sm[d] = s
            if s > best:
                best, bestd = s, d
        lanes.append((best, bestd))

    def period_better(x, y):
        (b2, d2), (best, bestd) = x, y
        return b2 > best or (b2 == best and d2 < bestd)
    best, bestd = _merge(lanes, (-1, INT_MAX), period_better)
    if best < K['CCS_MIN_SUPPORT']:
        return none
    p0 = bestd
    for q in range(2, 9):
        c = (bestd + q // 2) // q
        if c < DMIN:
            break
        es, eb = -1, -1
        for e in range(max(c - 3, DMIN), min(c + 3, dmax) + 1):
            if sm[e] > es:
                es, eb = sm[e], e
        if eb >= 0 and 2 * es >= best:
            p0 = eb
    # copy boundaries
    tol = max(p0 // 8, 4)
    W = min(p0, 96)
    dlo = p0 - tol

    def vote_better(x, y):
        (s2, e2, t2), (bs, bdel, bdist) = x, y
        return s2 > bs or (s2 == bs and (t2 < bdist or (t2 == bdist and e2 < bdel)))

    def closer(x, y):
        (d2, i2, a2, e2), (d1, i1_, a1, e1) = x, y
        return d2 < d1 or (d2 == d1 and (i2 > i1_ or (i2 == i1_ and (a2 < a1 or (a2 == a1 and e2 < e1)))))
    b, prev, cuts = 0, p0, []
    while len(cuts) < K['CCS_MAX_CUTS']:
        dhi = min(p0 + tol, L - b)
        if dhi < dlo:
            break
        nd = dhi - dlo + 1
        i0, i1 = max(b - W, 0), min(b + W, L)
        dh = [0] * nd
        for i in range(i0, i1):
            if next_[i] == -2:
                continue
            ci = code[i]
            j = head[(ci ^ (ci >> 5)) & (nbuckets - 1)]
            while j >= 0:                               # from the head: partners on both sides are in the chain
                delta = j - i
                if dlo <= delta <= dhi and code[j] == ci:
                    dh[delta - dlo] += 1
                j = next_[j]
        lanes = []
        for lane in range(NT):
            bs, bdel, bdist = -1, 0, INT_MAX
            for t in range(lane, nd, NT):
                delta = dlo + t
                sc = dh[t]
                dist = abs(delta - prev)
                if sc > bs or (sc == bs and dist < bdist):
                    bs, bdel, bdist = sc, delta, dist
            lanes.append((bs, bdel, bdist))
        bs, bdel, bdist = _merge(lanes, (-1, 0, INT_MAX), vote_better)
        if bs > 0:
            glo, ghi = max(bdel - GUARD, dlo), min(bdel + GUARD, dhi)
            lanes = []
            for lane in range(NT):
                mine = (INT_MAX, -1, INT_MAX, INT_MAX)
                for i in range(i0 + lane, i1, NT):
                    if next_[i] == -2:
                        continue
                    ci = code[i]
                    dist = abs(i + k // 2 - b)
                    if dist > mine[0]:
                        continue
                    j = head[(ci ^ (ci >> 5)) & (nbuckets - 1)]
                    while j >= 0:
                        delta = j - i
                        if glo <= delta <= ghi and code[j] == ci:
                            cand = (dist, i, abs(delta - prev), delta)
                            if closer(cand, mine):
                                mine = cand
                        j = next_[j]
                lanes.append(mine)
            bdel = _merge(lanes, (INT_MAX, -1, INT_MAX, INT_MAX), closer)[3]
        b += bdel
        prev = bdel
        cuts.append(b)
    if len(cuts) < 2:
        return none
    return p0, len(cuts), best, cuts


def segments(L, rec, K=None):
    """the copies K3 (poa_kernel_body) takes from a record: one per cut, and the rest of the read where it is long enough and the
    scan did not stop at its cap"""
    K = K or constants()
    period, ncuts, _support, cuts = rec
    if not period:
        return []
    out, b = [], 0
    for c in cuts[:ncuts]:
        out.append((b, c))
        b = c
    tail = L - b >= K['CCS_MIN_TAIL'] and ncuts < K['CCS_MAX_CUTS']
    if tail:
        out.append((b, L))
    return out


def cost(seq, nbuckets, K=None):
    """chain steps of the period count for this read at this number of buckets (what the model's time goes with)"""
    K = K or constants()
    seq = [int(x) for x in seq]
    k = K['CCS_K']
    fill = {}
    for i in range(len(seq) - k + 1):
        c = 0
        for b in seq[i:i + k]:
            if b < 0 or b > 3:
                break
            c = (c << 2) | b
        else:
            h = (c ^ (c >> 5)) & (nbuckets - 1)
            fill[h] = fill.get(h, 0) + 1
    return sum(n * (n - 1) // 2 for n in fill.values())
