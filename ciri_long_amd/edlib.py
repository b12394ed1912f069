"""Counterpart of the ``edlib`` Python module (edlib.align / edlib.getNiceAlignment), as CIRI-long and long-read tools call it
(CIRI_long/utils.py:153-159 uses the NW distance; adapter, primer and junction-probe searches use the HW mode).

    align(query, target, mode="NW", task="distance", k=-1, additionalEqualities=None) -> dict
    align_batch(queries, targets, ...) -> [dict]          (one batched GPU call)
    search(probes, texts, k=-1, both_strands=False, ...) -> array   (every probe in every text, HW, one batched GPU call)
    getNiceAlignment(result, query, target, gapSymbol="-") -> dict   (host only)

The result dict has edlib's keys: ``editDistance``, ``alphabetLength``, ``locations`` (a list of (start, end), both
inclusive and 0-based; start None for task "distance") and ``cigar`` (extended ops =, X, I, D; task "path" only).
Letters are raw bytes: ``str`` is encoded as latin-1, any byte value is allowed.  Unit costs.

Modes: NW aligns the whole query to the whole target, SHW to a prefix of the target, HW to any substring.  End locations are
every target column where the last query row reaches the best score, ascending; column -1 (the query before the target)
is a candidate for HW, and for every mode when the target is empty.  Starts: 0 for NW and SHW; for HW, an SHW pass of the
reversed query over the reversed target[0..end] and start = end - p for the last optimal position p (the longest alignment);
for an empty query, start = end + 1.  The CIGAR is the NW alignment of the query against target[start..end] of the first
location, traced back from the end cell preferring I (query letter against nothing), then D (target letter against
nothing), then the diagonal.  Distances, end locations and alphabetLength are uniquely defined; HW starts and CIGARs follow
the tie rules above (parity with edlib itself is unpinned: tests/golden/make_edlib_golden.py records it where edlib runs).

The kernels are K4m / K4t (csrc/edit_align.hip) through clh_edit_align_batch, and K4s (csrc/edit_search.hip) through
clh_edit_search_batch for search(); there is no CPU fallback.
"""
import numpy as np

from . import hip

_OPS = {7: '=', 8: 'X', 1: 'I', 2: 'D'}


def _as_bytes(s):
    if isinstance(s, str):
        return s.encode('latin-1')
    return bytes(s)


def cigar_string(ops):
    """BAM uint32 ops (len << 4 | op) -> extended CIGAR text, e.g. '3=1I'"""
    return ''.join('%d%s' % (int(o) >> 4, _OPS[int(o) & 0xf]) for o in ops)


def _check_args(mode, task, additionalEqualities):
    if mode not in hip.EA_MODES:
        raise ValueError('mode must be one of "NW", "SHW", "HW", got %r' % (mode,))
    if task not in hip.EA_TASKS:
        raise ValueError('task must be one of "distance", "locations", "path", got %r' % (task,))
    eq = []
    for pair in additionalEqualities or ():
        if len(pair) != 2:
            raise ValueError('additionalEqualities holds pairs of letters, got %r' % (pair,))
        a, b = (_as_bytes(x) if not isinstance(x, int) else bytes([x]) for x in pair)
        if len(a) != 1 or len(b) != 1:
            raise ValueError('additionalEqualities holds pairs of single letters, got %r' % (pair,))
        eq.append((a[0], b[0]))
    return eq


def results_from_rows(rows, locs, cig, task):
    out = []
    for r in rows:
        loc = [(None if task == 'distance' else int(s), int(e)) for s, e in locs[int(r['loc_off']):int(r['loc_off']) + int(r['nlocs'])]]
        cigar = None
        if task == 'path' and int(r['distance']) >= 0:
            cigar = cigar_string(cig[int(r['cigar_off']):int(r['cigar_off']) + int(r['cigar_len'])])
        out.append({'editDistance': int(r['distance']), 'alphabetLength': int(r['alphabet_len']), 'locations': loc, 'cigar': cigar})
    return out


def align_batch(queries, targets, mode='NW', task='distance', k=-1, additionalEqualities=None, context=None, workspace_bytes=0):
    """align() of every pair (queries[i], targets[i]) in one batched GPU call -> list of dicts"""
    eq = _check_args(mode, task, additionalEqualities)
    if len(queries) != len(targets):
        raise ValueError('align_batch: queries and targets differ in length')
    if not queries:
        return []
    ctx = context or hip.default_context()
    rows, locs, cig = ctx.edit_align_batch([_as_bytes(q) for q in queries], [_as_bytes(t) for t in targets], mode, task, int(k), eq,
                                           workspace_bytes)
    return results_from_rows(rows, locs, cig, task)


def align(query, target, mode='NW', task='distance', k=-1, additionalEqualities=None):
    """edlib.align with edlib's signature and result dict (see the module text)"""
    return align_batch([query], [target], mode, task, k, additionalEqualities)[0]


def search(probes, texts, k=-1, both_strands=False, additionalEqualities=None, context=None):
    """Every probe in every text: the cross product of align(probe, text, mode="HW", task="locations", k=k,
    additionalEqualities=...) in one batched GPU call, probes and texts uploaded once -> numpy structured array of shape
    (len(texts), len(probes), 2 if both_strands else 1) with the int32 fields

        distance   r["editDistance"] (-1: above k)
        start, end r["locations"][0]
        last_end   the end of r["locations"][-1]
        nlocs      len(r["locations"])

    of that call's result r; start, end and last_end are -2 when there is no location.  Slot [t, p, 0] is probes[p], slot
    [t, p, 1] is utils.revcomp(probes[p]) (bytes taken as latin-1).  The tie rules of the module text hold unchanged.
    additionalEqualities are applied to the letters as given on both strands: they are not complemented.
    Probes of 1..64 letters run on K4s (csrc/edit_search.hip: one wave per (probe, text) cell, its lanes on 64 column segments
    of the text).  Longer probes are answered in the same call through the pair route: their cross product goes to
    Context.edit_align_batch.  Empty probes and empty texts get align's answers."""
    eq = _check_args('HW', 'locations', additionalEqualities)
    from . import utils
    pb = []
    for p in probes:
        pb.append(_as_bytes(p))
        if both_strands:
            pb.append(utils.revcomp(pb[-1].decode('latin-1')).encode('latin-1'))
    tb = [_as_bytes(t) for t in texts]
    ns = 2 if both_strands else 1
    out = np.zeros((len(tb), len(pb)), dtype=hip.EDIT_SEARCH_DTYPE)
    if not tb or not pb:
        return out.reshape(len(tb), len(probes), ns)
    ctx = context or hip.default_context()
    short = [i for i, p in enumerate(pb) if len(p) <= 64]
    wide = [i for i, p in enumerate(pb) if len(p) > 64]
    if short:
        out[:, short] = ctx.edit_search_batch([pb[i] for i in short], tb, int(k), eq)
    if wide:
        rows, locs, _ = ctx.edit_align_batch([pb[i] for _ in tb for i in wide], [t for t in tb for _ in wide], 'HW', 'locations', int(k), eq)
        rows = rows.reshape(len(tb), len(wide))
        n, at = rows['nlocs'].astype(np.int64), rows['loc_off'].astype(np.int64)
        some = n > 0
        first, last = np.where(some, at, 0), np.where(some, at + n - 1, 0)
        sub = np.zeros(rows.shape, dtype=hip.EDIT_SEARCH_DTYPE)
        sub['distance'], sub['nlocs'] = rows['distance'], rows['nlocs']
        pad = np.concatenate([locs.reshape(-1, 2), np.full((1, 2), -2, dtype=np.int32)])
        sub['start'] = np.where(some, pad[first, 0], -2)
        sub['end'] = np.where(some, pad[first, 1], -2)
        sub['last_end'] = np.where(some, pad[last, 1], -2)
        out[:, wide] = sub
    return out.reshape(len(tb), len(probes), ns)


def getNiceAlignment(alignResult, query, target, gapSymbol='-'):
    """edlib.getNiceAlignment: the first location's alignment as three rows of equal length -- query_aligned,
    matched_aligned ('|' match, '.' mismatch, gapSymbol gap), target_aligned.  Host only."""
    cigar = alignResult.get('cigar')
    if cigar is None or not alignResult.get('locations'):
        raise ValueError('getNiceAlignment needs the result of align(..., task="path") with at least one location')
    qs = query.decode('latin-1') if isinstance(query, (bytes, bytearray)) else query
    ts = target.decode('latin-1') if isinstance(target, (bytes, bytearray)) else target
    start = alignResult['locations'][0][0] or 0
    qi, ti = 0, start
    qa, ma, ta = [], [], []
    num = ''
    for ch in cigar:
        if ch.isdigit():
            num += ch
            continue
        n, num = int(num), ''
        for _ in range(n):
            if ch in '=X':
                qa.append(qs[qi]); ta.append(ts[ti]); ma.append('|' if ch == '=' else '.')
                qi += 1; ti += 1
            elif ch == 'I':
                qa.append(qs[qi]); ta.append(gapSymbol); ma.append(gapSymbol)
                qi += 1
            elif ch == 'D':
                qa.append(gapSymbol); ta.append(ts[ti]); ma.append(gapSymbol)
                ti += 1
            else:
                raise ValueError('unknown CIGAR op %r' % ch)
    return {'query_aligned': ''.join(qa), 'matched_aligned': ''.join(ma), 'target_aligned': ''.join(ta)}
