"""K7 on the CPU: the checker tests/seed_check.py against the definitions it is written from (window enumeration, an all-pairs chain DP,
the bijection of the mix), and the __host__ __device__ functions of csrc/seed_device.h against the checker: tests/seed_host.hip is a
program of its own, built with AddressSanitizer and UBSan linked into it alone, that prints its inputs and answers.  No GPU is touched."""
import os
import random
import re
import shutil
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import seed_check as sc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which('hipcc') or ('/opt/rocm/bin/hipcc' if os.path.exists('/opt/rocm/bin/hipcc') else None)


def test_sketch_equals_window_enumeration():
    rng = random.Random(11)
    cases = 0
    for alpha in (2, 4, 5):
        for _ in range(120):
            k, w, n = rng.randint(4, 7), rng.randint(1, 8), rng.randint(1, 60)
            codes = [rng.randrange(alpha) for _ in range(n)]
            if rng.random() < 0.2 and n > 8:                     # a run of N
                a = rng.randrange(n)
                b = min(n, a + rng.randint(1, 10))
                codes[a:b] = [4] * (b - a)
            assert sc.sketch(codes, k, w) == sc.sketch_windows(codes, k, w), (alpha, k, w, codes)
            cases += 1
    assert cases == 360


def test_sketch_edges():
    assert sc.sketch([], 4, 3) == [] and sc.sketch([0, 1, 2], 4, 3) == []
    assert sc.sketch([0, 1, 2, 3], 4, 3) == []                   # ACGT is its own reverse complement
    homo = sc.sketch([0] * 20, 5, 4)
    assert [p for p, _, _ in homo] == list(range(16)) and len({key for _, key, _ in homo}) == 1      # every position ties
    assert len({key for _, key, _ in sc.sketch([0, 1] * 15, 5, 3)}) <= 2                             # a dinucleotide repeat: two keys
    fwd = sc.encode('ACGGTCATTGCAGGTACCATGACGTTAGC')
    a, b = sc.sketch(fwd, 7, 4), sc.sketch(sc.revcomp(fwd), 7, 4)
    assert sorted((len(fwd) - 7 - p, key, 1 - s) for p, key, s in b) == sorted(a)                    # the sketch is strand-symmetric


def test_mix_is_a_bijection():
    assert sorted(sc.mix(h, 4) for h in range(256)) == list(range(256))
    rng = random.Random(5)
    for k in (15, 28):
        xs = {rng.getrandbits(2 * k) for _ in range(100000)}
        ys = {sc.mix(h, k) for h in xs}
        assert len(ys) == len(xs) and max(ys) < 1 << (2 * k)


def _random_segment(rng, n):
    seg = set()
    while len(seg) < n:
        d = rng.choice((0, 0, 37, 900))
        x = rng.randrange(0, 3000)
        seg.add((x + d, max(0, x + rng.randint(-12, 12))))
    return sorted(seg)


def test_chain_dp_equals_all_pairs():
    rng = random.Random(3)
    for _ in range(150):
        n, k = rng.randint(0, 40), rng.choice((7, 15, 21))
        seg = _random_segment(rng, n)
        contig_of = lambda x: 0 if x < 2000 else 1                # noqa: E731
        f, p = sc.chains(seg, contig_of, k, lookback=64, max_gap=400, max_skew=30)
        assert f == sc.chains_all_pairs(seg, contig_of, k, max_gap=400, max_skew=30)
        for i in range(n):
            assert -1 <= p[i] < i and (f[i] == k) == (p[i] == -1)
            if p[i] >= 0:
                j = p[i]
                assert contig_of(seg[i][0]) == contig_of(seg[j][0])
                assert f[i] == f[j] + sc.gain(seg[i][0] - seg[j][0], seg[i][1] - seg[j][1], k)


def test_extraction_terminates_and_never_reuses_an_anchor():
    rng = random.Random(8)
    for _ in range(150):
        n, k = rng.randint(0, 60), 15
        seg = _random_segment(rng, n)
        f, p = sc.chains(seg, lambda x: 0, k, lookback=rng.choice((1, 3, 64)), max_gap=400, max_skew=30)
        max_chains, max_attempts = rng.randint(1, 5), rng.randint(1, 12)
        got, truncated = sc.extract(seg, f, p, k, min_score=rng.choice((15, 25, 40)), min_anchors=rng.randint(1, 3), max_chains=max_chains,
                                    max_attempts=max_attempts)
        assert len(got) <= min(max_chains, max_attempts)
        seen = set()
        for score, count, first, last in got:
            walk, i = [], last
            while i >= 0 and i not in seen and len(walk) < count:
                walk.append(i)
                i = p[i]
            assert len(walk) == count and walk[-1] == first and not seen & set(walk)
            seen |= set(walk)
        assert isinstance(truncated, bool)


@pytest.mark.skipif(HIPCC is None, reason='hipcc is not installed')
def test_device_header_functions_equal_the_checker_under_sanitizers(tmp_path):
    exe = str(tmp_path / 'seed_host')
    build = subprocess.run([HIPCC, '--offload-arch=gfx950', '-std=c++17', '-O1', '-g', '-Xarch_host', '-fsanitize=address,undefined',
                            '-I', os.path.join(ROOT, 'ciri_long_amd', 'csrc'), os.path.join(ROOT, 'tests', 'seed_host.hip'), '-o', exe],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run(['timeout', '-k', '10', '120', exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert 'runtime error' not in run.stderr, run.stderr              # UBSan reports and goes on
    lines = run.stdout.splitlines()
    m = re.match(r'^seed_host: (\d+) lines: ok$', lines[-1])
    assert m and int(m.group(1)) == len(lines) - 1, lines[-1]
    seqs, mins, counts = {}, {}, {'mix': 0, 'gain': 0}
    for line in lines[:-1]:
        t = line.split(' ')
        if t[0] == 'mix':
            assert sc.mix(int(t[2]), int(t[1])) == int(t[3]), line
            counts['mix'] += 1
        elif t[0] == 'gain':
            assert sc.gain(int(t[1]), int(t[2]), int(t[3])) == int(t[4]), line
            counts['gain'] += 1
        elif t[0] == 'seq':
            seqs[int(t[1])] = (int(t[2]), int(t[3]), [int(c) for c in t[4]])
        else:
            assert t[0] == 'min', line
            mins.setdefault(int(t[1]), []).append((int(t[2]), int(t[3]), int(t[4])))
    assert counts == {'mix': 180, 'gain': 400} and len(seqs) == 240
    for c, (k, w, codes) in seqs.items():
        assert mins.get(c, []) == sc.sketch(codes, k, w), (c, k, w, codes)
    assert sum(1 for v in mins.values() if v) > 100
