"""Host-side rules of bench.py that must hold without a GPU."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_gpus_n_under_a_profiler_refuses_to_spawn(monkeypatch):
    """under rocprofv3 the preloaded tool library has initialised the GPU, so `--gpus N` must not start
    child processes from this one; it has to exit non-zero before any Popen"""
    import bench
    monkeypatch.setenv('ROCPROFILER_TEST_MARK', '1')
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '2', '--steps', '1', '--warmup', '0'])
    called = []
    monkeypatch.setattr(subprocess, 'Popen', lambda *a, **k: called.append(a) or (_ for _ in ()).throw(AssertionError('Popen called')))
    monkeypatch.setattr(bench, 'launch_ranks', lambda n: called.append(n) or 0)
    with pytest.raises(SystemExit) as ei:
        bench.main()
    assert called == []
    assert ei.value.code not in (0, None) and 'profiler' in str(ei.value.code)


def test_profiler_detection_reads_the_preload_variables(monkeypatch):
    import bench
    for k in list(os.environ):
        if k.startswith('ROCPROF'):
            monkeypatch.delenv(k)
    for k in ('LD_PRELOAD', 'ROCP_TOOL_LIBRARIES', 'HSA_TOOLS_LIB'):
        monkeypatch.delenv(k, raising=False)
    assert not bench.under_profiler()
    monkeypatch.setenv('LD_PRELOAD', '/opt/rocm/lib/librocprofiler-sdk-tool.so')
    assert bench.under_profiler()


def _main_until_the_gpu(monkeypatch, argv):
    """bench.main() up to the point where it needs a GPU, with the CPU leg and the worker pool recorded instead of run"""
    import bench
    import torch
    for k in list(os.environ):
        if k.startswith('ROCPROF'):
            monkeypatch.delenv(k)
    for k in ('LD_PRELOAD', 'ROCP_TOOL_LIBRARIES', 'HSA_TOOLS_LIB', 'WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'CLH_BENCH_SPAWN'):
        monkeypatch.delenv(k, raising=False)
    called = []
    monkeypatch.setattr(bench, 'cpu_baseline', lambda seconds, wl: called.append(('cpu_baseline', seconds, wl)) or None)
    monkeypatch.setattr(bench, 'prepare_stage2_pool', lambda: called.append(('prepare_stage2_pool',)) or None)
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    monkeypatch.setattr(sys, 'argv', ['bench.py'] + argv)
    with pytest.raises(SystemExit) as ei:
        bench.main()
    assert 'needs a GPU' in str(ei.value.code)
    return called


def test_a_plain_run_starts_no_cpu_leg_and_no_worker_pool(monkeypatch):
    """`bench.py --gpus 1 --steps N --warmup W` does only what the headline figure needs: the CPU baseline and the forked workers of
    the extra lines belong to --full"""
    assert _main_until_the_gpu(monkeypatch, ['--gpus', '1', '--steps', '3', '--warmup', '1']) == []
    assert _main_until_the_gpu(monkeypatch, ['--gpus', '1', '--workload', 'c2']) == []


def test_full_runs_the_cpu_leg_and_prepares_the_extra_lines(monkeypatch):
    got = _main_until_the_gpu(monkeypatch, ['--gpus', '1', '--steps', '3', '--warmup', '1', '--full'])
    assert got == [('cpu_baseline', 12.0, 'c3'), ('prepare_stage2_pool',)]
    assert _main_until_the_gpu(monkeypatch, ['--full', '--no-cpu', '--no-extra']) == []
    assert _main_until_the_gpu(monkeypatch, ['--full', '--workload', 'c2', '--cpu-seconds', '2']) == [('cpu_baseline', 2.0, 'c2')]
