"""The plain statement of K7 (minimizer index, seeds, chains) over lists of base codes 0..4: the one yardstick of tests/test_gpu_seed.py
and tests/test_seed_host.py.  Written from the definitions of include/ciri_long_hip.h with no cleverness; every result is independent of
the order in which positions are visited, so a parallel kernel has to give the same lists."""


def encode(text):
    """letters -> codes: A/a 0, C/c 1, G/g 2, T/t 3, anything else 4"""
    return ['ACGT'.index(c) if c in 'ACGT' else 4 for c in text.upper()]


def revcomp(codes):
    return [3 - c if c < 4 else 4 for c in reversed(codes)]


def mix(h, k):
    m = (1 << (2 * k)) - 1
    h = (~h + (h << 21)) & m
    h ^= h >> 24
    h = (h + (h << 3) + (h << 8)) & m
    h ^= h >> 14
    h = (h + (h << 2) + (h << 4)) & m
    h ^= h >> 28
    h = (h + (h << 31)) & m
    return h


def pack(codes):
    v = 0
    for c in codes:
        v = v * 4 + c
    return v


def keys(codes, k):
    """per position 0..n-k: (key, strand), or None where there is no valid k-mer"""
    out = []
    for p in range(len(codes) - k + 1):
        word = codes[p:p + k]
        if any(c > 3 for c in word):
            out.append(None)
            continue
        f, r = pack(word), pack([3 - c for c in reversed(word)])
        out.append(None if f == r else (mix(min(f, r), k), int(f > r)))
    return out


def sketch_windows(codes, k, w):
    """the definition: p is selected iff it is valid and some window of w' positions inside [0, P) holds p and no valid key below key[p]"""
    ks = keys(codes, k)
    P = len(ks)
    if P <= 0:
        return []
    wp = min(w, P)
    chosen = set()
    for s in range(P - wp + 1):
        valid = [ks[q][0] for q in range(s, s + wp) if ks[q] is not None]
        if valid:
            low = min(valid)
            chosen.update(q for q in range(s, s + wp) if ks[q] is not None and ks[q][0] == low)
    return [(p, ks[p][0], ks[p][1]) for p in sorted(chosen)]


def selected(ks, p, wp):
    """the per-position rule: the runs a (left) and b (right) of positions whose key is invalid or >= key[p], clipped to the sequence"""
    if ks[p] is None:
        return False
    a = 0
    while a < wp and p - a - 1 >= 0 and (ks[p - a - 1] is None or ks[p - a - 1][0] >= ks[p][0]):
        a += 1
    b = 0
    while b < wp and p + b + 1 < len(ks) and (ks[p + b + 1] is None or ks[p + b + 1][0] >= ks[p][0]):
        b += 1
    return a + b + 1 >= wp


def sketch(codes, k, w):
    """[(position, key, strand)] by position"""
    ks = keys(codes, k)
    if not ks:
        return []
    wp = min(w, len(ks))
    return [(p, ks[p][0], ks[p][1]) for p in range(len(ks)) if selected(ks, p, wp)]


def index(contigs, k, w):
    """contigs: lists of codes, concatenated in order -> [(key, genome-wide position, strand)] sorted by (key, position)"""
    out, base = [], 0
    for ctg in contigs:
        out += [(key, base + p, s) for p, key, s in sketch(ctg, k, w)]
        base += len(ctg)
    return sorted(out)


def seeds(idx, read, k, w, max_occ):
    """-> (anchors [(minus, x, y)] ascending, repetitive)"""
    by_key = {}
    for key, pos, s in idx:
        by_key.setdefault(key, []).append((pos, s))
    anchors, repetitive = [], 0
    for q, key, s in sketch(read, k, w):
        hits = by_key.get(key, [])
        if len(hits) > max_occ:
            repetitive += 1
            continue
        for x, sg in hits:
            minus = s ^ sg
            anchors.append((minus, x, len(read) - k - q if minus else q))
    return sorted(anchors), repetitive


def beta(d, k):
    return 0 if d <= 0 else (k * d + 99) // 100 + (d.bit_length() - 1) // 2


def gain(dx, dy, k):
    return min(dx, dy, k) - beta(abs(dx - dy), k)


def admissible(xi, yi, xj, yj, same_contig, max_gap, max_skew):
    dx, dy = xi - xj, yi - yj
    return same_contig and dx > 0 and dy > 0 and dx <= max_gap and dy <= max_gap and abs(dx - dy) <= max_skew


def chains(seg, contig_of, k, lookback=64, max_gap=5000, max_skew=500):
    """seg: the anchors (x, y) of one (read, strand) in ascending order -> (f, p)"""
    f, p = [], []
    for i, (xi, yi) in enumerate(seg):
        best, arg = k, -1
        for j in range(i - 1, max(i - lookback, 0) - 1, -1):
            xj, yj = seg[j]
            if admissible(xi, yi, xj, yj, contig_of(xi) == contig_of(xj), max_gap, max_skew):
                v = f[j] + gain(xi - xj, yi - yj, k)
                if v > best:
                    best, arg = v, j
        f.append(best)
        p.append(arg)
    return f, p


def chains_all_pairs(seg, contig_of, k, max_gap=5000, max_skew=500):
    """the same f over every earlier anchor, for lookback >= the segment: the maximum alone, no p"""
    f = []
    for i, (xi, yi) in enumerate(seg):
        cand = [f[j] + gain(xi - seg[j][0], yi - seg[j][1], k) for j in range(i)
                if admissible(xi, yi, seg[j][0], seg[j][1], contig_of(xi) == contig_of(seg[j][0]), max_gap, max_skew)]
        f.append(max([k] + cand))
    return f


def extract(seg, f, p, k, min_score=40, min_anchors=3, max_chains=4, max_attempts=None):
    """-> ([(score, count, first index, last index)], truncated)"""
    if max_attempts is None:
        max_attempts = 8 * max_chains
    used = [False] * len(seg)
    out, attempts, truncated = [], 0, False
    while len(out) < max_chains:
        free = [i for i in range(len(seg)) if not used[i]]
        if not free:
            break
        e = min(free, key=lambda i: (-f[i], i))
        if f[e] < min_score:
            break
        if attempts >= max_attempts:
            truncated = True
            break
        attempts += 1
        i, count, first = e, 0, e
        while i >= 0 and not used[i]:
            used[i] = True
            count += 1
            first = i
            i = p[i]
        score = f[e] - (f[i] if i >= 0 else 0)
        if score >= min_score and count >= min_anchors:
            out.append((score, count, first, e))
    return out, truncated


class Genome(object):
    """contigs [(name, text)] as the checker sees them"""

    def __init__(self, contigs):
        self.names = [n for n, _ in contigs]
        self.codes = [encode(t) for _, t in contigs]
        self.start, at = [], 0
        for c in self.codes:
            self.start.append(at)
            at += len(c)
        self.end = at

    def contig_of(self, x):
        return max(c for c in range(len(self.start)) if self.start[c] <= x)


def read_chains(genome, idx, read, k, w, max_occ, lookback=64, max_gap=5000, max_skew=500, min_score=40, min_anchors=3, max_chains=4,
                max_attempts=None):
    """-> (chains of the read as SeedIndex.chains gives them, [truncated plus, truncated minus])"""
    anchors, _ = seeds(idx, read, k, w, max_occ)
    out, trunc = [], []
    for minus in (0, 1):
        seg = [(x, y) for m, x, y in anchors if m == minus]
        f, p = chains(seg, genome.contig_of, k, lookback, max_gap, max_skew)
        got, t = extract(seg, f, p, k, min_score, min_anchors, max_chains, max_attempts)
        trunc.append(t)
        for score, count, first, last in got:
            c = genome.contig_of(seg[last][0])
            out.append({'minus': minus, 'contig': c, 'score': score, 'anchors': count, 'x_first': seg[first][0] - genome.start[c], 'y_first': seg[first][1],
                        'x_end': seg[last][0] - genome.start[c] + k, 'y_end': seg[last][1] + k})
    return sorted(out, key=lambda c: (-c['score'], c['minus'], c['x_first'])), trunc


def map_read(genome, idx, read, k, w, max_occ, **params):
    """what seed.map_reads gives for one read"""
    got, _ = read_chains(genome, idx, read, k, w, max_occ, **params)
    L, rows = len(read), []
    for c in got:
        name = genome.names[c['contig']]
        if c['minus']:
            qs, qe, anchor = L - c['y_end'], L - c['y_first'], (name, c['x_first'] + k, L - k - c['y_first'])
        else:
            qs, qe, anchor = c['y_first'], c['y_end'], (name, c['x_first'], c['y_first'])
        rows.append({'contig': name, 'minus': bool(c['minus']), 'score': c['score'], 'anchors': c['anchors'], 'ref_start': c['x_first'], 'ref_end': c['x_end'],
                     'query_start': qs, 'query_end': qe, 'anchor': anchor})
    return rows
