"""bench.py's host-side pieces without a GPU: --dump-outputs' files and size bound, and the --steps check."""
import os
import subprocess
import sys

import numpy as np
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _out(B=64, T=10, K=101):
    g = torch.Generator().manual_seed(0)
    full = torch.randn(B, T, K, generator=g)
    valid = torch.rand(B, T, generator=g) < 0.8
    logits = torch.randn(B, K, generator=g)
    return dict(full_logits=full, valid_masks=valid, logits=logits, probs=logits.softmax(-1),
                scale=torch.tensor(100.0, dtype=torch.float64), note='not an array')


def test_dump_writes_every_array_whole_under_the_limit(tmp_path):
    out = _out()
    got = bench.dump_outputs(out, str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == ['full_logits.npy', 'logits.npy', 'probs.npy', 'scale.npy', 'valid_masks.npy']
    assert got['full_logits'] == ([64, 10, 101], 64) and got['scale'] == ([], None)
    for name in ('full_logits', 'logits', 'probs'):
        x = np.load(tmp_path / f'{name}.npy')
        assert x.dtype == np.float32
        np.testing.assert_array_equal(x, out[name].numpy())
    m = np.load(tmp_path / 'valid_masks.npy')
    assert m.dtype == np.float32 and np.array_equal(m, out['valid_masks'].numpy().astype(np.float32))
    s = np.load(tmp_path / 'scale.npy')
    assert s.dtype == np.float64 and s.shape == () and s.item() == 100.0


def test_dump_samples_the_same_rows_within_the_limit(tmp_path):
    """Above the limit every array keeps the same seeded rows, whatever the values: two builds write comparable files."""
    out = _out()
    limit = 200_000
    a, b = tmp_path / 'a', tmp_path / 'b'
    bench.dump_outputs(out, str(a), limit=limit)
    other = {k: (v + 1 if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in out.items()}
    got = bench.dump_outputs(other, str(b), limit=limit)
    assert sum(os.path.getsize(p) for p in a.iterdir()) <= limit
    rows = got['full_logits'][1]
    assert 0 < rows < 64 and got['logits'][1] == rows
    full = out['full_logits'].numpy()
    sa, sb = np.load(a / 'full_logits.npy'), np.load(b / 'full_logits.npy')
    assert sa.shape == (rows, 10, 101)
    idx = [int(np.nonzero((full == r).all(axis=(1, 2)))[0][0]) for r in sa]      # the rows are rows of the output, in order
    assert idx == sorted(set(idx))
    np.testing.assert_array_equal(sb, sa + 1)
    np.testing.assert_array_equal(np.load(a / 'logits.npy'), out['logits'].numpy()[idx])


def _extras(monkeypatch, argv, world=1):
    monkeypatch.setattr(sys, 'argv', ['bench.py'] + argv)
    return bench.extras(bench.parse(), world)


def test_a_plain_run_measures_nothing_behind_the_timed_steps(monkeypatch):
    """Only --full adds measurements after the timed region; an explicit --from-host stays on in any run."""
    every = {'value_from_host', 'dvfs', 'tolerance_mode', 'ms_per_step_strict', 'cpu_baseline', 'other_configs'}
    assert _extras(monkeypatch, []) == set()
    assert _extras(monkeypatch, ['--config', '3', '--no-dvfs']) == set()
    assert _extras(monkeypatch, ['--from-host']) == {'value_from_host'}
    assert _extras(monkeypatch, ['--full']) == every
    assert _extras(monkeypatch, ['--full', '--gpus', '2'], world=2) == set()
    assert _extras(monkeypatch, ['--full', '--from-host', '--gpus', '2'], world=2) == {'value_from_host'}
    for flag, key in (('--no-from-host', 'value_from_host'), ('--no-dvfs', 'dvfs'), ('--no-tolerance-mode', 'tolerance_mode'),
                      ('--no-strict-line', 'ms_per_step_strict'), ('--no-cpu-baseline', 'cpu_baseline'),
                      ('--no-other-configs', 'other_configs')):
        assert _extras(monkeypatch, ['--full', flag]) == every - {key}, flag
    # the other configs and the lines of their own carry no headline-only measurement
    assert _extras(monkeypatch, ['--full', '--config', '3']) == {'dvfs', 'ms_per_step_strict', 'cpu_baseline'}
    for own in (['--precise'], ['--precise-blocks', '2'], ['--tolerance-mode']):
        assert _extras(monkeypatch, ['--full'] + own) == every - {'tolerance_mode', 'other_configs'}, own
    assert _extras(monkeypatch, ['--full', '--f16-weights']) == every - {'other_configs'}


def test_steps_below_one_is_refused():
    for bad in (['--steps', '0'], ['--warmup', '-1']):
        r = subprocess.run([sys.executable, 'bench.py'] + bad, cwd=ROOT, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and '--steps must be >= 1' in r.stderr, r.stderr[-2000:]
