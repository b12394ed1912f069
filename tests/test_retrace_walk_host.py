"""The resumable walk of K1g's recompute route on the CPU, under AddressSanitizer and UBSan: tests/retrace_host.hip is a program of its
own that includes csrc/ssw_pairs.h and feeds pr_walk_round tile after tile with slices of random planes, each tile buffer exactly as
large as the kernels' guard (EnKept) computes: 6 000 cases of one to five chunks for each of the three gap models, held to pr_walk over
EnCells on the whole plane -- rows, ops and EN_ST_NO_WALK verdicts -- and some with a damaged record.  What it asserts is stated at
its top.  The sanitizers are linked into that program alone; no GPU is touched."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which('hipcc') or ('/opt/rocm/bin/hipcc' if os.path.exists('/opt/rocm/bin/hipcc') else None)


@pytest.mark.skipif(HIPCC is None, reason='hipcc is not installed')
def test_the_resumed_walk_equals_the_whole_walk_on_random_planes_under_sanitizers(tmp_path):
    exe = str(tmp_path / 'retrace_host')
    build = subprocess.run([HIPCC, '--offload-arch=gfx950', '-std=c++17', '-O1', '-g', '-Xarch_host', '-fsanitize=address,undefined',
                            '-I', os.path.join(ROOT, 'ciri_long_amd', 'csrc'), os.path.join(ROOT, 'tests', 'retrace_host.hip'), '-o', exe],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run(['timeout', '-k', '10', '120', exe], capture_output=True, text=True)
    print(run.stdout + run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    assert 'runtime error' not in run.stderr, run.stderr              # UBSan reports and goes on
    m = re.search(r'^retrace_host: 3 models, (\d+) cases, (\d+) walked, (\d+) refused, (\d+) resumed, (\d+) records damaged: ok$', run.stdout, re.M)
    assert m, run.stdout
    cases, walked, refused, resumed, damaged = map(int, m.groups())
    assert cases == 18000 and walked + refused == cases and walked > 1000 and resumed > 3000 and damaged > 100
