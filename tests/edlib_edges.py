"""Seeded edlib.align cases at the edges where K4m / K4t (csrc/edit_align.hip, planned by clh_edit_align_plan_create in
csrc/clh_api.hip) are most likely to be wrong (not a test module): every lane-group class G = 1 .. 64 with and without idle lanes,
two to four passes of 64 blocks through the ping-pong carry buffers, reverse-pass slots beyond one launch, additionalEqualities
over eight bit planes, the 8 / 9 letter switch of the planes, the feeder's 16-byte look-ahead at short targets, the k bound and
workspace chunks.  tests/test_edlib_edges_host.py holds the CPU statements (model against checker, the edges are reached) and
tests/test_gpu_edlib_edges.py the kernels.

A batch is a Batch tuple (queries, targets, mode, task, k, equalities, workspace_bytes); all_cases() returns named lists of them.
Everything is drawn from random.Random(seed).  The plan's routing is restated below in plain Python (ea_group, blocks, passes,
ea_pad, the reverse-launch slot count, the workspace bytes and chunks), so that the tests can assert that a set reaches what it is
named for without a GPU."""
import collections
import random

MODES = ('NW', 'SHW', 'HW')
TASKS = ('path', 'locations', 'distance')         # path first: expected() derives the other two tasks from it
DNA = b'ACGT'
AA20 = b'ACDEFGHIKLMNPQRSTVWY'

Batch = collections.namedtuple('Batch', 'queries targets mode task k equalities workspace_bytes')

CLASS_LENGTHS = (64, 65, 128, 129, 256, 257, 512, 513, 577, 1024, 1025, 2048, 2049, 2113, 4095, 4096)
PASS_LENGTHS = (4097, 8191, 8192, 8193, 8257, 12289)
FEEDER_N = (1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65)
FEEDER_M = (1, 64, 65, 300, 1100, 4097)


# ---- the plan's routing, restated ------------------------------------------------------------------------------------------
def blocks(m):
    return (m + 63) >> 6


def ea_group(m):
    """lanes per pair: the power of two that holds the blocks, at most 64"""
    G = 1
    while G < blocks(m) and G < 64:
        G <<= 1
    return G


def passes(m):
    return max(1, (blocks(m) + 63) >> 6)


def idle_lanes(m):
    return ea_group(m) - min(blocks(m), 64)


def ea_pad(n):
    return ((n + 63) & ~63) + 64


REV_CARRY_BYTES = 256 << 20


def rev_launch_slots(pairs):
    """slots per reverse-pass launch of a lane-group class that holds `pairs` [(m, n)]; None when no pair of it has carry buffers"""
    pmax = max([min(n, 2 * m + 1) for m, n in pairs if m > 4096], default=0)
    return max(1, REV_CARRY_BYTES // (2 * ea_pad(pmax))) if pmax else None


def path_bytes(m, n, mode):
    """workspace of one pair's K4t task: 20 bytes per block and column of the longest target[start..end], rounded up to 256"""
    lmax = n if mode == 'NW' else min(n, 2 * m)
    return (20 * blocks(m) * lmax + 255) & ~255


def workspace_chunks(batch):
    """the chunks clh_edit_align_plan_create cuts a path batch into: pairs in input order while they fit the limit -> [[(m, n)]]"""
    limit = batch.workspace_bytes or (1 << 30)
    out, used = [], 0
    for q, t in zip(batch.queries, batch.targets):
        if not q or not t:
            continue
        b = path_bytes(len(q), len(t), batch.mode)
        if not out or used + b > limit:
            out.append([]); used = 0
        out[-1].append((len(q), len(t))); used += b
    return out


def letters(batch):
    return len(set(b''.join(batch.queries)) | set(b''.join(batch.targets)))


# ---- sequences ---------------------------------------------------------------------------------------------------------------
def rand_seq(rng, n, alpha):
    return bytes(rng.choice(alpha) for _ in range(n))


def mutate(rng, s, rate, alpha):
    """substitutions, deletions and insertions, a third of `rate` each"""
    out = bytearray()
    for ch in s:
        r = rng.random()
        if r < rate / 3:
            out.append(rng.choice(alpha))
        elif r < 2 * rate / 3:
            continue
        elif r < rate:
            out.append(ch); out.append(rng.choice(alpha))
        else:
            out.append(ch)
    return bytes(out)


def planted(rng, m, alpha, rate, flank):
    """a query of exactly m letters and a target that holds a copy of it mutated at `rate` inside random flanks of 0..flank"""
    q = rand_seq(rng, m, alpha)
    return q, rand_seq(rng, rng.randint(0, flank), alpha) + mutate(rng, q, rate, alpha) + rand_seq(rng, rng.randint(0, flank), alpha)


def tandem(rng, m, alpha):
    """a tandem-repeat query of m letters (substitutions only, so m holds) in a pure repeat a little longer: ties and several ends"""
    unit = rand_seq(rng, rng.randint(2, 6), alpha)
    q = bytearray((unit * (m // len(unit) + 1))[:m])
    for _ in range(rng.choice([0, 1, m // 50])):
        q[rng.randrange(m)] = rng.choice(alpha)
    return bytes(q), (unit * (m // len(unit) + 20))[:m + rng.randint(0, 40)]


def unrelated(rng, m, alpha):
    return rand_seq(rng, m, alpha), rand_seq(rng, rng.randint(max(1, m // 2), m + 100), alpha)


def _batches(qs, ts, tasks=TASKS, modes=MODES, eq=None, ws=0):
    return [Batch(list(qs), list(ts), mode, task, -1, eq, ws) for mode in modes for task in tasks]


# ---- 1. lane-group classes -----------------------------------------------------------------------------------------------------
def class_pairs(alpha, seed):
    """a planted, a tandem-repeat and an unrelated pair per length of CLASS_LENGTHS, shuffled (the plan sorts by class; results
    come back in input order), with empty queries and empty targets in between"""
    rng = random.Random(seed)
    pairs = []
    for m in CLASS_LENGTHS:
        pairs += [planted(rng, m, alpha, rng.choice([0, 0.05, 0.1, 0.2]), 200), tandem(rng, m, alpha), unrelated(rng, m, alpha)]
    rng.shuffle(pairs)
    for at, pair in ((3, (b'', rand_seq(rng, 30, alpha))), (11, (rand_seq(rng, 700, alpha), b'')), (20, (b'', b'')),
                     (31, (b'', rand_seq(rng, 2000, alpha))), (len(pairs), (rand_seq(rng, 5, alpha), b''))):
        pairs.insert(at, pair)
    return [q for q, _ in pairs], [t for _, t in pairs]


def classes():
    return _batches(*class_pairs(DNA, 101)) + _batches(*class_pairs(AA20, 102))


# ---- 2. passes -----------------------------------------------------------------------------------------------------------------
def pass_short_pairs(seed=201):
    """queries of PASS_LENGTHS against two targets of 1..400 letters each (one shorter than the 64 lanes' skew), cut from the query"""
    rng = random.Random(seed)
    qs, ts = [], []
    for m in PASS_LENGTHS:
        q = rand_seq(rng, m, DNA)
        for n in (rng.randint(1, 63), rng.randint(64, 400)):
            a = rng.randrange(m - n)
            qs.append(q); ts.append(mutate(rng, q[a:a + n], 0.1, DNA)[:n] or b'A')
    return qs, ts


def pass_long_pairs(seed=202):
    """queries of PASS_LENGTHS against planted targets of about m + 0..700 letters"""
    rng = random.Random(seed)
    pairs = [planted(rng, m, DNA, 0.03, 350) for m in PASS_LENGTHS]
    return [q for q, _ in pairs], [t for _, t in pairs]


def pass_path_8193(seed=203):
    """8193 x about 8400, HW, path: three passes in the score pass, the reverse pass and K4t.  The full checker's path needs the whole
    m x n matrix (0.55 GB, twice that while numpy builds it), so this one result is held to edlib_check.check_invariants and
    check_locations (a valid CIGAR of exactly the optimal cost over target[start..end], the smallest start) and to the checker's
    'locations' result, not to the checker's own CIGAR."""
    q, t = planted(random.Random(seed), 8193, DNA, 0.03, 100)
    return Batch([q], [t], 'HW', 'path', -1, None, 0)


def passes_short():
    return _batches(*pass_short_pairs(), tasks=('path',))


def passes_long():
    return _batches(*pass_long_pairs(), tasks=('locations',))


# ---- 3. reverse launches -------------------------------------------------------------------------------------------------------
def homopolymer(rng, m, n, x):
    """query A * m with x letters replaced by C, target A * n"""
    q = bytearray(b'A' * m)
    for p in rng.sample(range(m), x):
        q[p] = ord('C')
    return bytes(q), b'A' * n


def homopolymer_closed_form(m, n, x, mode='HW'):
    """HW of that family (n >= m): x of the query's letters never match, and any window of m - x .. m target letters costs exactly x
    (a C is an insertion or a mismatch); the longest window that ends at `end` has m letters, or starts at column 0"""
    assert mode == 'HW' and n >= m >= x
    return {'editDistance': x, 'alphabetLength': 2 if x else 1,
            'locations': [(max(0, e - m + 1), e) for e in range(m - 1 - x, n)], 'cigar': None}


REVERSE_HOMOPOLYMER = (4097, 22000, 3)     # m, n, x


def reverse_launches(seed=301):
    """HW, locations, one batch -> (batch, index of the random long pair, index of the homopolymer pair, index of the G = 64 pair
    without carry buffers).  Both long pairs have more slots (n + 1) than one reverse launch of their class holds."""
    rng = random.Random(seed)
    q1 = rand_seq(rng, 4200, DNA)
    t1 = rand_seq(rng, 17000 - 4300, DNA) + mutate(rng, q1, 0.03, DNA)
    t1 += rand_seq(rng, 17000 - len(t1), DNA)             # the copy ends about 100 columns before the target does
    pairs = [planted(rng, 40, DNA, 0.1, 60), (q1, t1), planted(rng, 300, DNA, 0.05, 100), planted(rng, 3000, DNA, 0.03, 250),
             homopolymer(rng, *REVERSE_HOMOPOLYMER), planted(rng, 90, DNA, 0.1, 30)]
    return Batch([q for q, _ in pairs], [t for _, t in pairs], 'HW', 'locations', -1, None, 0), 1, 4, 3


# ---- 4. additionalEqualities over eight planes -----------------------------------------------------------------------------------
IUPAC = {'R': 'AG', 'Y': 'CT', 'S': 'GC', 'W': 'AT', 'K': 'GT', 'M': 'AC', 'B': 'CGT', 'D': 'AGT', 'H': 'ACT', 'V': 'ACG', 'N': 'ACGT'}
EQ_LENGTHS = (50, 200, 1000, 2500, 4200)     # G = 1, 4, 16, 64 and two passes


def _eq_pairs(rng, plain, codes, rate):
    """planted pairs of EQ_LENGTHS over `plain`; a letter of the query or of the copy becomes one of `codes` at `rate`"""
    def sprinkle(s):
        return bytes(rng.choice(codes) if rng.random() < rate else c for c in s)
    qs, ts = [], []
    for m in EQ_LENGTHS:
        q, t = planted(rng, m, plain, 0.06, 80)
        qs.append(sprinkle(q)); ts.append(sprinkle(t))
    return qs, ts


def eq_protein(seed=401):
    """the 20 amino acids, B = {D, N}, Z = {E, Q}, J = {I, L}, X = every other letter (23 partners)"""
    rng = random.Random(seed)
    eq = [(ord('B'), ord('D')), (ord('B'), ord('N')), (ord('Z'), ord('E')), (ord('Z'), ord('Q')), (ord('J'), ord('I')), (ord('J'), ord('L'))]
    eq += [(ord('X'), c) for c in AA20 + b'BZJ']
    eq += [(ord('B'), ord('D')), (ord('D'), ord('B')), (ord('K'), ord('K')), (ord('U'), ord('C'))]   # duplicate, reversed, self, absent letter
    return _batches(*_eq_pairs(rng, AA20, b'BZJX', 0.08), tasks=('path',), eq=eq)


def eq_bytes(seed=402):
    """all 256 byte values; 0xff equals every other byte, 0x00 equals 0x80..0x9f (every letter is in the batch, so none is absent)"""
    rng = random.Random(seed)
    eq = [(0xff, c) for c in range(255)] + [(0, c) for c in range(0x80, 0xa0)]
    eq += [(0xff, 7), (7, 0xff), (9, 9)]
    qs, ts = _eq_pairs(rng, bytes(range(1, 255)), b'\x00\xff', 0.08)
    qs.append(bytes(range(256))); ts.append(bytes(reversed(range(256))))
    return _batches(qs, ts, tasks=('path',), eq=eq)


def eq_bytes_absent(seed=404):
    """the byte set without 0xfe: 255 letters, codes above 127 among them, and equalities that name the absent byte, which drop out"""
    rng = random.Random(seed)
    eq = [(0xff, c) for c in range(254)] + [(0, c) for c in range(0x80, 0xa0)]
    eq += [(0xfe, 0x90), (0xc8, 0xfe), (0xfe, 0xfe), (0xff, 200), (200, 0xff), (9, 9)]
    qs, ts = _eq_pairs(rng, bytes(range(1, 254)), b'\x00\xff', 0.08)
    qs.append(bytes(range(254)) + b'\xff'); ts.append(bytes(reversed(range(254))) + b'\xff')
    return _batches(qs, ts, tasks=('path',), eq=eq)


def eq_iupac(seed=403):
    """IUPAC DNA, 15 letters with their standard sets; the last pair is (A, C): N = A and N = C do not make A = C"""
    rng = random.Random(seed)
    eq = [(ord(c), ord(b)) for c, bases in sorted(IUPAC.items()) for b in bases]
    eq += [(ord('N'), ord('A')), (ord('A'), ord('N')), (ord('G'), ord('G')), (ord('U'), ord('T'))]
    qs, ts = _eq_pairs(rng, DNA, ''.join(sorted(IUPAC)).encode(), 0.08)
    return _batches(qs + [b'A'], ts + [b'C'], tasks=('path',), eq=eq)


# ---- 5. eight and nine letters -------------------------------------------------------------------------------------------------
EIGHT = b'ACGTNRYK'
EIGHT_EQ = [(ord(c), ord(b)) for c in 'NRYK' for b in IUPAC[c]]


def eight_and_nine(seed=501):
    """-> [(batch of exactly 8 letters, the same batch and one pair that brings a ninth)], without and with equalities, per mode"""
    rng = random.Random(seed)
    pairs = [planted(rng, m, EIGHT, 0.1, 60) for m in (1, 20, 64, 65, 129, 300, 600, 1100)]
    pairs += [tandem(rng, 200, EIGHT), unrelated(rng, 90, EIGHT)]
    qs, ts = [q for q, _ in pairs], [t for _, t in pairs]
    q9, t9 = planted(rng, 150, EIGHT + b'W', 0.1, 60)
    out = []
    for eq in (None, EIGHT_EQ):
        for mode in MODES:
            out.append((Batch(qs, ts, mode, 'path', -1, eq, 0), Batch(qs + [q9], ts + [t9], mode, 'path', -1, eq, 0)))
    return out


# ---- 6. the feeder -------------------------------------------------------------------------------------------------------------
def feeder(seed=601):
    """one batch per (mode, n): queries of FEEDER_M against targets of exactly n letters, so the last pair's target -- as long as any
    in the batch -- ends the symbol buffer and its 16-byte look-ahead reads the padding.  In HW every optimal end has a reverse task
    whose reversed view starts n - 1 - end bytes into the reversed target."""
    rng = random.Random(seed)
    out = []
    for n in FEEDER_N:
        qs, ts = [], []
        for m in FEEDER_M:
            q = rand_seq(rng, m, DNA)
            a = rng.randrange(max(1, m - n))
            t = mutate(rng, (q[a:a + n] + rand_seq(rng, n, DNA))[:n], 0.15, DNA)
            qs.append(q); ts.append((t + rand_seq(rng, n, DNA))[:n])
        out += _batches(qs, ts, tasks=('path',))
    return out


# ---- 7. k ----------------------------------------------------------------------------------------------------------------------
def k_pairs():
    """-> [(query, target, tasks)]: the planted DNA pair of every class, every short-target pair of the pass set (locations and
    path), every long-target pair of the pass set (locations: the checker's path would need the whole matrix) and an identical pair.
    k_batches() takes d from the checker and makes the calls k = d, k = d - 1, k = 0 and k = m + 1 of them."""
    rng = random.Random(701)
    out = [planted(rng, m, DNA, rng.choice([0.05, 0.1, 0.2]), 100) + (('path', 'locations'),) for m in CLASS_LENGTHS]
    out += [(q, t, ('path', 'locations')) for q, t in zip(*pass_short_pairs())]
    out += [(q, t, ('locations',)) for q, t in zip(*pass_long_pairs())]
    q = rand_seq(rng, 700, DNA)
    out.append((q, q, ('path', 'locations')))
    return out


_best = {}


def k_batches(check, modes=MODES):
    """-> [(Batch of one pair with its k, the checker's free distance d)]: k = d keeps the free result, k = d - 1 leaves the empty
    one, k = 0 keeps an identical pair only, k = m + 1 keeps everything.  d is the checker's (edlib_check.ends_of), once per pair
    and mode."""
    out = []
    for q, t, tasks in k_pairs():
        for mode in modes:
            if (q, t, mode) not in _best:
                _best[q, t, mode] = check.ends_of(check._arr(q), check._arr(t), mode, check.eq_matrix())[0]
            d = _best[q, t, mode]
            out += [(Batch([q], [t], mode, task, k, None, 0), d) for task in tasks for k in sorted({d, d - 1, 0, len(q) + 1}) if k >= 0]
    return out


# ---- 8. workspace --------------------------------------------------------------------------------------------------------------
def workspace(seed=801):
    """-> (a HW path batch under a limit that cuts it into chunks of several lane-group classes each, a single NW pair, its bytes b)"""
    rng = random.Random(seed)
    pairs = [planted(rng, m, DNA, 0.1, 150) for m in (100, 577, 300, 1100, 64, 1025, 513, 129, 900, 200, 700, 65)]
    limit = 640 << 10
    q, t = planted(rng, 777, DNA, 0.1, 100)
    return Batch([q for q, _ in pairs], [t for _, t in pairs], 'HW', 'path', -1, None, limit), (q, t), path_bytes(len(q), len(t), 'NW')


def plan_batch():
    """HW, path, every class of the DNA class set and one pair of two passes: run twice on one plan"""
    qs, ts = class_pairs(DNA, 101)
    q, t = planted(random.Random(901), 4200, DNA, 0.05, 120)
    return Batch(qs + [q], ts + [t], 'HW', 'path', -1, None, 0)


def all_cases():
    """name -> [Batch]: exactly the batches the two test modules run (they take them from here or from the same builders;
    tests/test_edlib_edges_host.py test_all_cases_are_the_builders keeps the two in step).  Every batch is held to the full checker
    result by result, except the homopolymer pair of 'reverse_launches' (closed form) and 'passes_path_8193' (invariants; see
    pass_path_8193).  The k set asks the checker (tests/edlib_check.py) for its distances."""
    import edlib_check
    ws_batch, (q, t), b = workspace()
    return collections.OrderedDict([
        ('classes', classes()),
        ('passes_short', passes_short()),
        ('passes_long', passes_long()),
        ('passes_path_8193', [pass_path_8193()]),
        ('reverse_launches', [reverse_launches()[0]]),
        ('eq_protein', eq_protein()),
        ('eq_bytes', eq_bytes()),
        ('eq_bytes_absent', eq_bytes_absent()),
        ('eq_iupac', eq_iupac()),
        ('eight_and_nine', [b9 for _, b9 in eight_and_nine()]),
        ('feeder', feeder()),
        ('k', [b_ for b_, _ in k_batches(edlib_check)]),
        ('workspace', [ws_batch, Batch([q], [t], 'NW', 'path', -1, None, b)]),
        ('plan', [plan_batch()]),
    ])


# ---- the checker's answers, computed once per process ----------------------------------------------------------------------------
_memo = {}


def expected(check, q, t, mode, task, k=-1, eq=None):
    """edlib_check.align(q, t, mode, task, k, eq).  The free result is computed once per (pair, mode) and task: 'locations' is
    'path' without its CIGAR and 'distance' is 'locations' without its starts (edlib_check.align computes them in that order),
    and the k rule is the checker's own (edlib_check.bounded)."""
    key = (q, t, mode, tuple(eq) if eq else None)
    have = _memo.setdefault(key, {})
    if task not in have:
        if task == 'path':
            have['path'] = check.align(q, t, mode, 'path', -1, eq)
        elif 'locations' not in have:
            have['locations'] = dict(have['path'], cigar=None) if 'path' in have else check.align(q, t, mode, 'locations', -1, eq)
        if task == 'distance':
            have['distance'] = dict(have['locations'], cigar=None, locations=[(None, e) for _, e in have['locations']['locations']])
    return check.bounded(have[task], k)
