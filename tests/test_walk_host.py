"""The walk-back of K1g and K1gb on the CPU, under AddressSanitizer and UBSan: tests/walk_host.hip is a program of its own that includes
csrc/ssw_pairs.h, whose walk (pr_walk) and cell locators (EnCells, BdCells) are __host__ __device__, and runs them over planes of
random bytes, exactly as large as the walk kernels' guards compute: 20 000 cases for each of the five (geometry, model) pairs, and for
every model a gap state that reaches column 0 and one that reaches row 0.  What it asserts is stated at its top.  The sanitizers are
linked into that program alone; no GPU is touched."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which('hipcc') or ('/opt/rocm/bin/hipcc' if os.path.exists('/opt/rocm/bin/hipcc') else None)


@pytest.mark.skipif(HIPCC is None, reason='hipcc is not installed')
def test_walk_on_random_planes_under_sanitizers(tmp_path):
    exe = str(tmp_path / 'walk_host')
    build = subprocess.run([HIPCC, '--offload-arch=gfx950', '-std=c++17', '-O1', '-g', '-Xarch_host', '-fsanitize=address,undefined',
                            '-I', os.path.join(ROOT, 'ciri_long_amd', 'csrc'), os.path.join(ROOT, 'tests', 'walk_host.hip'), '-o', exe],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run(['timeout', '-k', '10', '120', exe], capture_output=True, text=True)
    print(run.stdout + run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    assert 'runtime error' not in run.stderr, run.stderr              # UBSan reports and goes on
    m = re.search(r'^walk_host: 5 instantiations, (\d+) cases, (\d+) walked, (\d+) refused, (\d+) boundary cases refused: ok$', run.stdout, re.M)
    assert m, run.stdout
    cases, walked, refused, boundary = map(int, m.groups())
    assert cases == 100000 and walked + refused == cases and walked > 0 and boundary == 24
