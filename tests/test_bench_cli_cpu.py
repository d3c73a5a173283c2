"""The plain `bench.py --gpus 1 --steps K --warmup W` run and `--dump-outputs DIR`, on the CPU with the emulated ops
(DEVA_BENCH_EMULATED=1) and a tiny frame: the contract line, K timed steps, and the last step's outputs written the
same way by two runs of the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(tmp_path, tag, *extra):
    env = dict(os.environ, DEVA_BENCH_EMULATED='1', OMP_NUM_THREADS='2', DEVA_BENCH_EXTRA_DIR=str(tmp_path))
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    out_dir = tmp_path / tag
    res = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1',
                          '--height', '96', '--width', '128', '--objects', '2', '--dump-outputs', str(out_dir), *extra],
                         env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    return json.loads(res.stdout.rstrip('\n').splitlines()[-1]), out_dir


def test_plain_run_line_and_dumped_outputs(tmp_path):
    line, a = _bench(tmp_path, 'a')
    assert line['steps'] == 3 and line['warmup'] == 1 and line['unit'] == 'frames/s' and line['higher_is_better'] is True
    assert line['dtype'] == 'f32' and line['metric'].startswith('propagation FPS @480p')
    assert line['value'] > 0 and abs(line['value'] - 1e3 / line['ms_per_step']) < 1e-4 * line['value']
    # the measurements of --full are not taken by a plain run
    assert not {'roofline', 'cpu_baseline'} & set(line)
    with open(tmp_path / 'bench_extra.json') as f:
        assert not {'also', 'affinity', 'also_kernels', 'timed_like_eval_vos'} & set(json.load(f))
    prob = np.load(a / 'prob.npy')
    assert prob.dtype == np.float32 and prob.shape == (3, 96, 128)             # background + 2 objects
    assert np.allclose(prob.sum(0), 1.0, atol=1e-4)
    _, b = _bench(tmp_path, 'b')
    assert sorted(os.listdir(a)) == sorted(os.listdir(b)) == ['prob.npy']
    assert np.array_equal(prob, np.load(b / 'prob.npy'))


def test_dump_outputs_samples_large_outputs_with_a_fixed_seed(tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(bench, 'DUMP_BYTES', 40000)
    g = torch.Generator().manual_seed(0)
    arrays = {'big': torch.rand(2, 100, 100, generator=g), 'wide': torch.rand(50, 100, generator=g, dtype=torch.float64)}
    bench.dump_outputs(str(tmp_path / 'a'), arrays)
    bench.dump_outputs(str(tmp_path / 'b'), arrays)
    total = 0
    for name in arrays:
        x, y = np.load(tmp_path / 'a' / f'{name}.npy'), np.load(tmp_path / 'b' / f'{name}.npy')
        assert np.array_equal(x, y) and x.dtype == arrays[name].numpy().dtype and x.ndim == 1
        assert np.isin(x, arrays[name].numpy().reshape(-1)).all()
        total += x.nbytes
    assert total <= 40000


def test_headline_clip_is_the_stream_then_runs_back_and_forth(monkeypatch):
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(bench, 'HEADLINE_DISTINCT_FRAMES', 4)
    stream = bench.make_clip(16, 16, 4, seed=3, device='cpu')
    clip = bench.make_headline_clip(16, 16, 11, seed=3, device='cpu')
    assert [next(i for i, s in enumerate(stream) if torch.equal(s, f)) for f in clip] == [0, 1, 2, 3, 2, 1, 0, 1, 2, 3, 2]
    assert all(torch.equal(a, b) for a, b in zip(bench.make_headline_clip(16, 16, 3, seed=3, device='cpu'), stream))
