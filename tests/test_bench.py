"""bench.py command-line contract: --dump-outputs and --full."""
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load_bench():
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        'heterofl_bench', os.path.join(ROOT, 'bench.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_dtypes_and_budget(tmp_path, monkeypatch):
    """dump_outputs writes float32/float64 .npy files; over the byte budget
    it stores the same seeded sample on every call."""
    bench = _load_bench()
    arrays = {'w': torch.arange(1000, dtype=torch.bfloat16).reshape(10, 100),
              'd': torch.arange(6, dtype=torch.float64),
              'n': torch.tensor([3, 1, 2])}
    bench.dump_outputs(str(tmp_path / 'a'), arrays)
    w = np.load(tmp_path / 'a' / 'w.npy')
    assert w.dtype == np.float32 and w.shape == (10, 100)
    assert np.array_equal(w, arrays['w'].float().numpy())
    assert np.load(tmp_path / 'a' / 'd.npy').dtype == np.float64
    n = np.load(tmp_path / 'a' / 'n.npy')
    assert n.dtype == np.float64 and n.tolist() == [3.0, 1.0, 2.0]
    # 3 arrays, 1200-byte budget: only 'w' (4000 B) exceeds its 400 B share
    monkeypatch.setattr(bench, 'DUMP_BUDGET_BYTES', 1200)
    bench.dump_outputs(str(tmp_path / 'b'), arrays)
    bench.dump_outputs(str(tmp_path / 'c'), arrays)
    wb = np.load(tmp_path / 'b' / 'w.npy')
    assert wb.shape == (100,) and wb.dtype == np.float32
    assert np.array_equal(wb, np.load(tmp_path / 'c' / 'w.npy'))
    assert set(wb.tolist()) <= set(w.reshape(-1).tolist())
    assert np.load(tmp_path / 'b' / 'n.npy').tolist() == [3.0, 1.0, 2.0]
    total = sum(os.path.getsize(tmp_path / 'b' / f)
                for f in os.listdir(tmp_path / 'b'))
    assert total <= 1200 + 3 * 128   # payload + .npy headers


def test_bench_full_and_dump_cli(tmp_path):
    """One tiny CPU run with --full --dump-outputs: the result line carries
    ms_per_step and the whole-round figure, and the last timed round's
    global parameters land in DIR as float arrays within 64 MB."""
    env = dict(os.environ, HETEROFL_BENCH_SPU='10', OMP_NUM_THREADS='2',
               CUDA_VISIBLE_DEVICES='', HIP_VISIBLE_DEVICES='')
    out_dir = tmp_path / 'dump'
    out = subprocess.run(
        [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1',
         '--steps', '1', '--warmup', '0', '--full',
         '--dump-outputs', str(out_dir)],
        cwd=str(tmp_path), capture_output=True, text=True, timeout=600,
        env=dict(env, PYTHONPATH=ROOT))
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, out.stdout
    rec = json.loads(lines[0])
    assert rec['steps'] == 1 and rec['ms_per_step'] > 0
    assert rec['round_ms_incl_stats'] > 0
    files = sorted(os.listdir(out_dir))
    assert 'active_users.npy' in files and len(files) > 10
    total = 0
    for f in files:
        a = np.load(out_dir / f)
        assert a.dtype in (np.float32, np.float64), f
        assert np.isfinite(a).all(), f
        total += a.nbytes
    assert total <= 64 * 1024 * 1024
    assert len(np.load(out_dir / 'active_users.npy')) == 10
