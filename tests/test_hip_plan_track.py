"""lg_plan_track on the GPU (k_plan_track): the fused launch against the same steps made one at a time
(lg_romsim_policy per model step, float32 torch for the model) on the bits, the reference's own tracking loop
(tests/golden/plan_track.npz) against the float64 restatement under the chain yardstick of section 10.2, the saturating plan, the
simulator's untouched state and the refusals."""
import json
import os

import numpy as np
import pytest
import torch

from tests import plan_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sim(model_dt, rom_dt=0.1, vel=0.3, acc=0.5, Kp=10.0, Kd=10.0, envs=4):
    from legged_gym_dev_amd.tube.rom_sim import HipRomSim, RomSimCfg
    rc = RomSimCfg()
    rc.env.num_envs, rc.env.model.dt, rc.rom.dt = envs, model_dt, rom_dt
    rc.env.model.z_min, rc.env.model.z_max = [-1e9, -1e9, -vel, -vel], [1e9, 1e9, vel, vel]
    rc.env.model.v_min, rc.env.model.v_max = [-acc, -acc], [acc, acc]
    rc.controller.Kp, rc.controller.Kd = Kp, Kd
    return HipRomSim(rc, seed=3, device=DEV)


def _plans(B, N, dt, seed):
    """Random plans whose inputs reach past the model's velocity bound, so that both of its bounds bind on some steps."""
    g = torch.Generator().manual_seed(seed)
    z0 = torch.rand(B, 2, generator=g) - 0.5
    v = 0.5 * (2 * torch.rand(B, N, 2, generator=g) - 1)
    z, dt = [z0], torch.tensor(dt, dtype=torch.float32)
    for k in range(N):
        z.append(z[-1] + dt * v[:, k])
    x0 = torch.cat([z0 + 0.05 * torch.randn(B, 2, generator=g), 0.1 * torch.randn(B, 2, generator=g)], dim=1)
    return torch.stack(z, dim=1), v, x0


def _stepwise(sim, z, v, x0, S, rom_dt):
    """The same steps one at a time: the host builds the observation, lg_romsim_policy gives the action, float32 torch applies f."""
    B, N = v.shape[:2]
    z, v = z.to(DEV), v.to(DEV)
    x = (torch.cat([z[:, 0], torch.zeros(B, 2, device=DEV)], dim=1) if x0 is None else x0.to(DEV)).clone()
    dt = torch.tensor(np.float32(sim.cfg.env.model.dt), device=DEV)
    xs, us = [x.clone()], []
    for t in range(N):
        ff = v[:, min(t + 1, N - 1)]
        for s in range(S):
            frac = torch.tensor((np.float32(s) * np.float32(sim.cfg.env.model.dt)) / np.float32(rom_dt), device=DEV)
            ref = z[:, t] + (z[:, t + 1] - z[:, t]) * frac
            a = sim.policy(torch.cat([x, ref, ff], dim=1))
            pos = x[:, :2] + dt * x[:, 2:]
            vel = x[:, 2:] + dt * a
            x = torch.cat([pos, vel], dim=1)
            us.append(a)
        xs.append(x.clone())
    xs = torch.stack(xs, dim=1)
    e = xs[:, :, :2] - z
    s2 = torch.zeros(B, N + 1, device=DEV)
    s2 = s2 + e[..., 0] * e[..., 0]
    s2 = s2 + e[..., 1] * e[..., 1]
    return {"x": xs, "u": torch.stack(us, dim=1), "pz_x": xs[:, :, :2].contiguous(), "w_true": torch.sqrt(s2)}


@pytest.mark.parametrize("N", [1, 7, 50])
@pytest.mark.parametrize("S", [1, 2])
def test_fused_launch_equals_the_stepwise_path(S, N):
    from legged_gym_dev_amd.tube.plan import track
    sim = _sim(0.1 / S)
    try:
        for B in (1, 63, 64, 65):
            z, v, x0 = _plans(B, N, 0.1, seed=100 * N + B)
            for start in (x0, None):
                got, want = track(sim, z, v, start), _stepwise(sim, z, v, start, S, 0.1)
                assert tuple(got["u"].shape) == (B, N * S, 2)
                for k in ("x", "u", "pz_x", "w_true"):
                    assert torch.equal(got[k], want[k]), f"{k}: S {S}, N {N}, B {B}, x0 {'given' if start is not None else 'from z'}"
                if B == 65 and N > 1:
                    u = got["u"].abs()
                    assert bool((u == 0.5).any()) and bool(((u < 0.5) & (u > 0)).any())      # bound and interior both occur
                if start is None:                                        # the optional outputs change nothing
                    only = track(sim, z, v, None, want=())
                    assert set(only) == {"pz_x", "w_true"}
                    assert torch.equal(only["pz_x"], got["pz_x"]) and torch.equal(only["w_true"], got["w_true"])
    finally:
        sim.close()


@pytest.fixture(scope="module")
def fx():
    z = np.load(os.path.join(ROOT, "tests", "golden", "plan_track.npz"))
    return {**{k: z[k] for k in ("z", "v", "x", "u", "w")}, "cfg": json.loads(str(z["meta_cfg"])), "names": json.loads(str(z["meta_names"]))}


@pytest.fixture(scope="module")
def fixture_runs(fx):
    """The reference's plans tracked by the device and by the restatement in float32 and float64, once for the tests below."""
    from legged_gym_dev_amd.tube.plan import track
    c = fx["cfg"]
    sim = _sim(c["model_dt"], c["model_dt"], vel=2.0, acc=2.0, Kp=c["Kp"], Kd=c["Kd"])
    try:
        got = {k: t.cpu().numpy() for k, t in track(sim, fx["z"], fx["v"], fx["x"][:, 0]).items()}
    finally:
        sim.close()
    z32, v32 = fx["z"].astype(np.float32), fx["v"].astype(np.float32)       # what the device is given
    ref = {D: plan_ref.track(c, z32, v32, x0=fx["x"][:, 0], S=1, rom_dt=c["model_dt"], dtype=D) for D in (np.float32, np.float64)}
    return got, ref


def test_reference_loop_within_the_chain_yardstick(fx, fixture_runs):
    """pz_x, x and u of the reference's 16 plans: e32 = max |float32 restatement - float64| per array, the device within 4 e32 (the
    margin of DESIGN.md section 10.2, for the same reason: a closed loop with gains of 10 on differences of nearby numbers).  The
    float64 restatement itself is the reference's run to the per-step bound (tests/test_plan_host.py)."""
    got, ref = fixture_runs
    for k in ("pz_x", "x", "u", "w_true"):
        r32, r64 = ref[np.float32][k].astype(np.float64), ref[np.float64][k]
        e32, ours = np.abs(r32 - r64).max(), np.abs(got[k].astype(np.float64) - r64).max()
        print(f"{k}: e32 = {e32:.3e}, device / e32 = {ours / e32 if e32 else 0:.2f}")
        assert ours <= 4 * e32 if e32 else ours == 0, (k, ours, e32)


def test_saturating_plan_sits_on_the_bounds_the_restatement_names(fx, fixture_runs):
    got, ref = fixture_runs
    assert fx["names"][-1] == "saturating"
    b32, b64 = ref[np.float32]["bind"][-1], ref[np.float64]["bind"][-1]
    agree = b32 == b64                                                   # the step where the bound changes may fall on either side
    assert agree.mean() > 0.9 and (np.abs(b64) == 1).any() and (np.abs(b64) == 2).any()
    u, x = got["u"][-1], got["x"][-1]
    acc = agree & (np.abs(b64) == 1)
    np.testing.assert_array_equal(u[acc], 2.0 * np.sign(b64[acc]).astype(np.float32))           # the acceleration bound itself
    vel = agree & (np.abs(b64) == 2)
    dt = np.float32(fx["cfg"]["model_dt"])
    bound = (np.float32(2.0) * np.sign(b64).astype(np.float32) - x[:-1, 2:]) / dt              # (z_max - xdot) / dt of the device's own state
    np.testing.assert_array_equal(u[vel], bound[vel])
    assert np.abs(x[:, 2:]).max() <= 2.0 + 1e-6


def test_the_simulator_is_not_touched():
    from legged_gym_dev_amd.tube.plan import track
    sim = _sim(0.05)
    try:
        sim.reset()
        sim.step(None)
        torch.cuda.synchronize()
        before = {k: sim.t[k].clone() for k in ("tg_state", "root_states", "tg_traj", "v_traj", "obs", "n_resample")}
        epoch = sim.lib.lg_romsim_get_epoch(sim.ctx)
        z, v, x0 = _plans(65, 7, 0.1, seed=1)
        track(sim, z, v, x0)
        torch.cuda.synchronize()
        for k, t in before.items():
            assert torch.equal(sim.t[k], t), k
        assert sim.lib.lg_romsim_get_epoch(sim.ctx) == epoch
    finally:
        sim.close()


def test_refusals():
    from legged_gym_dev_amd.lib import LeggedHipError
    from legged_gym_dev_amd.tube.plan import track
    sim = _sim(0.05)
    try:
        z, v, x0 = _plans(3, 4, 0.1, seed=2)
        with pytest.raises(LeggedHipError, match="rom_dt"):
            track(sim, z, v, x0, rom_dt=0.12)                           # 2.4 model steps per node
        with pytest.raises(LeggedHipError, match="S must be 1..8"):
            track(sim, z, v, x0, rom_dt=0.5)
        with pytest.raises(ValueError, match="z must be"):
            track(sim, z[:, :4], v, x0)
        with pytest.raises(ValueError, match="x0 must be"):
            track(sim, z, v, x0[:, :2])
        p = lambda t: None if t is None else __import__("ctypes").c_void_p(t.data_ptr())
        zd, vd = z.to(DEV), v.to(DEV)
        assert sim.lib.lg_plan_track(sim.ctx, p(zd), p(vd), None, 3, 4, 2, 0.1, None, None, None, None) == -1
        assert "missing array" in sim.lib.lg_last_error().decode()
        assert sim.lib.lg_plan_track(sim.ctx, p(zd), p(vd), None, 3, 65, 2, 0.1, None, None, None, None) == -1
        assert "N must be" in sim.lib.lg_last_error().decode()
    finally:
        sim.close()
