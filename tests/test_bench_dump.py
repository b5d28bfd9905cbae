"""bench.py --dump-outputs: what the last timed step computed, as DIR/<name>.npy, within the size budget and the same from run to run."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fake_run(N, T=24, O=48, A=12):
    g = torch.Generator().manual_seed(0)
    t = {k: torch.randn(T, N, O, generator=g) for k in ("obs", "critic_obs")}
    t.update({k: torch.randn(T, N, A, generator=g) for k in ("actions", "mu")})
    t.update({k: torch.randn(T, N, generator=g) for k in ("rewards", "values", "returns", "advantages", "log_prob")})
    t["dones"] = torch.randint(0, 2, (T, N), dtype=torch.uint8, generator=g)
    t["stats"] = torch.arange(1, 9, dtype=torch.float32)
    ppo = types.SimpleNamespace(t=t, privileged=False, N=N,
                                param_views={"std": torch.ones(A), "actor.0.weight": torch.randn(64, O, generator=g)})
    env = types.SimpleNamespace(obs_buf=torch.randn(N, O, generator=g), rew_buf=torch.randn(N, generator=g),
                                reset_buf=torch.zeros(N, dtype=torch.bool), privileged_obs_buf=None)
    return env, types.SimpleNamespace(ppo=ppo)


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_keeps_a_seeded_env_sample_within_the_budget(tmp_path):
    import bench
    env, runner = _fake_run(512)
    full = bench.dump_outputs(env, runner, str(tmp_path / "full"))
    assert full["envs_kept"] == 512 and not (tmp_path / "full" / "env_index.npy").exists()
    a = _load(tmp_path / "full")
    np.testing.assert_array_equal(a["storage_obs"], runner.ppo.t["obs"].numpy())
    np.testing.assert_array_equal(a["losses"], np.array([3 / 6, 4 / 6], np.float32))
    budget = full["bytes"] // 3
    outs = []
    for name in ("s1", "s2"):
        info = bench.dump_outputs(env, runner, str(tmp_path / name), budget=budget)
        assert 0 < info["envs_kept"] < 512 and info["bytes"] <= budget
        assert sum(os.path.getsize(tmp_path / name / f) for f in os.listdir(tmp_path / name)) == info["bytes"]
        outs.append(_load(tmp_path / name))
    s = outs[0]
    assert all(v.dtype in (np.float32, np.float64) for v in s.values())
    idx = s["env_index"].astype(np.int64)
    assert len(idx) == len(set(idx.tolist())) and list(idx) == sorted(idx)
    np.testing.assert_array_equal(s["storage_obs"], a["storage_obs"][:, idx])
    np.testing.assert_array_equal(s["env_obs"], a["env_obs"][idx])
    np.testing.assert_array_equal(s["param_actor.0.weight"], a["param_actor.0.weight"])        # no env axis: whole
    for k in s:
        np.testing.assert_array_equal(s[k], outs[1][k])                                       # the same sample every time


@pytest.mark.gpu
def test_bench_dump_outputs_repeat_bit_for_bit(tmp_path):
    """Two runs with the same arguments: the JSON line carries steps and ms_per_step, and the dumped arrays are identical."""
    dumps = []
    for r in range(2):
        d = tmp_path / f"run{r}"
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                            "--num_envs", "256", "--hidden", "64,32", "--no_other", "--no_alt", "--no_cpu_baseline", "--sustained", "0",
                            "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, p.stdout
        out = json.loads(lines[0])
        assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0
        assert out["dump_outputs"]["envs_kept"] == 256 and out["dump_outputs"]["deterministic"] is True
        assert out["dump_outputs"]["bytes"] == sum(os.path.getsize(d / f) for f in os.listdir(d)) <= 64 * 10 ** 6
        dumps.append(_load(d))
    a, b = dumps
    assert a["storage_obs"].shape == (24, 256, 48) and a["param_actor.0.weight"].shape == (64, 48)
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].dtype in (np.float32, np.float64), k
        assert np.isfinite(a[k]).all(), k
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
