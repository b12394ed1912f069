"""The gather of genome windows on the CPU, under AddressSanitizer and UBSan: tests/gather_host.hip is a program of its own that
includes csrc/genome_gather.h, whose index arithmetic, shift, byte reversal, packed decode and tail stores (gather_word,
gather_combine, gather_move_word) are __host__ __device__ and are all a lane of genome_gather_kernel runs.  It rebuilds windows at
every source offset mod 16, every length 0..70, lengths around one and two tiles, in all four flag values, from byte 0 and up to the
last byte of a genome array of exactly length + pad bytes, and compares them with a per-byte loop.  The sanitizers are linked into
that program alone; no GPU is touched."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which('hipcc') or ('/opt/rocm/bin/hipcc' if os.path.exists('/opt/rocm/bin/hipcc') else None)


@pytest.mark.skipif(HIPCC is None, reason='hipcc is not installed')
def test_gather_rebuilds_windows_under_sanitizers(tmp_path):
    exe = str(tmp_path / 'gather_host')
    build = subprocess.run([HIPCC, '--offload-arch=gfx950', '-std=c++17', '-O1', '-g', '-Xarch_host', '-fsanitize=address,undefined',
                            '-I', os.path.join(ROOT, 'ciri_long_amd', 'csrc'), os.path.join(ROOT, 'tests', 'gather_host.hip'), '-o', exe],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run(['timeout', '-k', '10', '120', exe], capture_output=True, text=True)
    print(run.stdout + run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    assert 'runtime error' not in run.stderr, run.stderr              # UBSan reports and goes on
    m = re.search(r'^gather_host: tile (\d+), (\d+) windows, (\d+) words: ok$', run.stdout, re.M)
    assert m, run.stdout
    tile, windows, words = map(int, m.groups())
    header = open(os.path.join(ROOT, 'ciri_long_amd', 'csrc', 'genome_gather.h')).read()
    assert tile == int(re.search(r'kGatherTile = (\d+);', header).group(1))
    # per genome and flag value: 71 lengths at 48 offsets and at the end, 6 lengths around the tile at 16 offsets and at the end, the
    # whole genome; a window without a letter has no tile, every other at least one of tile / 16 words
    assert windows == 16 * 4 * (71 * 49 + 6 * 17 + 1) and words >= (tile // 16) * (windows - 16 * 4 * 49)
