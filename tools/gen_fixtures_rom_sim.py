#!/usr/bin/env python3
"""Golden fixture of the ROM-on-ROM simulator: tests/golden/rom_sim_double_single.npz

TEST INFRASTRUCTURE -- needs the reference tree (REF of oracle/gen_fixtures.py); the .npz it writes is committed and holds data
only.  Drives the reference's own CustomSim (deep_tube_learning/custom_sim.py), DoubleInt2D / SingleInt2D / TrajectoryGenerator
(trajopt/rom_dynamics.py), samplers (deep_tube_learning/utils.py) and DoubleSingleTracking (deep_tube_learning/controllers.py) on
the CPU, imported by file path with the stand-in modules of oracle/gen_fixtures_trajectory.py::load_trajectory_modules.  The
collection loop (data_collection_trajectory.py:111-149) is restated here with one deliberate change: the first action of the epoch
uses the observation AFTER env.reset() (the reference keeps the one from before it, :94,111,137), as scripts/
collect_trajectory_data.py::collect does.

Every torch.rand / randint draw is recorded into per-env, per-event slots (include/legged_hip.h LG_RS_SLOT_*, then one block of 20
per generator resample of that env, torch.randint's value as itself).  The samplers' hard-coded device='cuda' is dropped by the
recorder (CPU run).

Configuration: double_single_int.yaml with 64 envs, T = 40 records, hold times 0.05..0.6 s (several resamples per env, some inside
the reset's N-step loop), prob_stationary 0.2.

    python tools/gen_fixtures_rom_sim.py
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, ROOT)
import gen_fixtures as gf  # noqa: E402
import gen_fixtures_trajectory as gft  # noqa: E402

N_ENVS, T, SEED, N_STATE = 64, 40, 7, 16
CFG = dict(N=10, dN=1, model_dt=0.05, rom_dt=0.1, Kp=10.0, Kd=10.0,
           model_z_min=[-1e9, -1e9, -0.3, -0.3], model_z_max=[1e9, 1e9, 0.3, 0.3], model_v_min=[-0.5, -0.5], model_v_max=[0.5, 0.5],
           rom_v_min=[-0.2, -0.2], rom_v_max=[0.2, 0.2], t_low=0.05, t_high=0.6, freq_low=0.01, freq_high=2.0, prob_stationary=0.2,
           weight_sampler="UniformWeightSamplerNoRamp", randomize_rom_distance=True, max_rom_dist=[1.0, 1.0], zero_rom_dist_llh=0.25,
           noise_lo=[0.0, 0.0, -0.1, -0.1], noise_hi=[0.0, 0.0, 0.1, 0.1])
TG_FIELDS = {"weights": (0, 4), "t_final": (4, 1), "t": (5, 1), "k": (6, 1), "sample_hold_input": (7, 2), "extreme_input": (9, 2),
             "ramp_t_start": (11, 1), "ramp_v_start": (12, 2), "ramp_v_end": (14, 2), "sin_mag": (16, 2), "sin_freq": (18, 2),
             "sin_off": (20, 2), "sin_mean": (22, 2), "stationary_inds": (24, 1), "v": (25, 2)}          # LG_TG_* offsets
TG_STRIDE = 30


def _ns(d):
    return types.SimpleNamespace(**{k: _ns(v) if isinstance(v, dict) else v for k, v in d.items()})


def sim_cfg():
    c = CFG
    return _ns(dict(
        env=dict(num_envs=N_ENVS, episode_length_s=T * c["rom_dt"],
                 model=dict(cls="DoubleInt2D", dt=c["model_dt"], z_min=c["model_z_min"], z_max=c["model_z_max"], v_min=c["model_v_min"],
                            v_max=c["model_v_max"])),
        rom=dict(cls="SingleInt2D", dt=c["rom_dt"], z_min=[-1e9, -1e9], z_max=[1e9, 1e9], v_min=c["rom_v_min"], v_max=c["rom_v_max"]),
        trajectory_generator=dict(cls="TrajectoryGenerator", t_samp_cls="UniformSampleHoldDT", weight_samp_cls=c["weight_sampler"],
                                  N=c["N"], t_low=c["t_low"], t_high=c["t_high"], freq_low=c["freq_low"], freq_high=c["freq_high"],
                                  seed=SEED, prob_stationary=c["prob_stationary"], dN=c["dN"]),
        domain_rand=dict(randomize_rom_distance=c["randomize_rom_distance"], max_rom_distance=c["max_rom_dist"],
                         zero_rom_dist_llh=c["zero_rom_dist_llh"]),
        init_state=dict(default_noise_lower=c["noise_lo"], default_noise_upper=c["noise_hi"])))


def load_by_path(fullname, rel):
    spec = importlib.util.spec_from_file_location(fullname, os.path.join(gf.REF, rel))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[fullname] = mod
    spec.loader.exec_module(mod)
    return mod


LOG = []


def install_recorder():
    orig_rand, orig_randint = torch.rand, torch.randint

    def rand(*a, **kw):
        kw.pop("device", None)
        out = orig_rand(*a, **kw)
        LOG.append(out.clone())
        return out

    def randint(*a, **kw):
        kw.pop("device", None)
        out = orig_randint(*a, **kw)
        LOG.append(out.clone().float())
        return out
    torch.rand, torch.randint = rand, randint


def tg_row(tg, n):
    row = np.zeros((n, TG_STRIDE), np.float32)
    for name, (off, w) in TG_FIELDS.items():
        row[:, off:off + w] = getattr(tg, name)[:n].detach().numpy().astype(np.float32).reshape(n, w)
    return row


def main():
    gf._build_isaacgym_stub(gf._STATE)
    gf._load_reference_modules()
    gft.load_trajectory_modules()
    rd = sys.modules["trajopt.rom_dynamics"]
    cs = load_by_path("deep_tube_learning.custom_sim", "deep_tube_learning/custom_sim.py")
    ct = load_by_path("deep_tube_learning.controllers", "deep_tube_learning/controllers.py")
    install_recorder()
    torch.manual_seed(SEED)
    n = N_ENVS
    resamples = [[] for _ in range(n)]
    orig_resample = rd.TrajectoryGenerator.resample

    def resample_spy(self, idx, z):
        if len(idx) == 0:
            return orig_resample(self, idx, z)
        start = len(LOG)
        orig_resample(self, idx, z)
        draws = LOG[start:]
        del LOG[start:]
        block = torch.cat([d.reshape(len(idx), -1).float() for d in draws], 1).numpy()
        assert block.shape[1] == 20, block.shape
        for j, e in enumerate(idx.tolist()):
            resamples[e].append(block[j])
    rd.TrajectoryGenerator.resample = resample_spy

    env = cs.CustomSim(sim_cfg())
    assert env.device.type == "cpu"
    policy = ct.DoubleSingleTracking(CFG["Kp"], CFG["Kd"], state_dependent_input_bound=env.model.clip_v_z)
    tg = env.traj_gen
    draw_reset = np.zeros((n, 9), np.float32)
    assert len(LOG) == 1 and tuple(LOG[0].shape) == (n, 2)
    draw_reset[:, 7:9] = LOG[0].numpy()
    del LOG[:]

    steps = []
    in_reset_loop = np.zeros(n, bool)

    def snap(obs, act, k_before, nres_before):
        nres = np.array([len(r) for r in resamples], np.int32)
        steps.append(dict(k=tg.k.numpy().copy(), t=tg.t.numpy().copy(), t_final=tg.t_final.numpy().copy(),
                          stationary=tg.stationary_inds.numpy().copy(), weights=tg.weights.numpy().copy(),
                          extreme=tg.extreme_input.numpy().copy(), nres=nres, stepped=tg.k.numpy() != k_before,
                          resampled=nres != nres_before, root=env.root_states.numpy().copy(), obs=obs.numpy().copy(),
                          act=act.numpy().copy(), tg_row=tg_row(tg, N_STATE), tg_traj=tg.trajectory[:N_STATE].numpy().copy(),
                          v_traj=tg.v_trajectory[:N_STATE].numpy().copy(), trajectory=env.trajectory[:N_STATE].numpy().copy()))

    # ---- the epoch (data_collection_trajectory.py:104-149, first action from the fresh observation)
    rom_n, x_n = env.rom.n, env.get_state().shape[1]
    x, z, pz_x = torch.zeros((n, T + 1, x_n)), torch.zeros((n, T + 1, rom_n)), torch.zeros((n, T + 1, rom_n))
    v, done = torch.zeros((n, T, env.rom.m)), torch.zeros((n, T), dtype=torch.bool)
    orig_step = env.step
    state = {"in_reset": True}

    def step_spy(action):                                  # counts of the reset loop: taken just before the reset's own step
        if state["in_reset"]:
            in_reset_loop[:] = np.array([len(r) for r in resamples]) > 1
            state["k0"], state["n0"] = tg.k.numpy().copy(), np.array([len(r) for r in resamples], np.int32)
            state["in_reset"] = False
        return orig_step(action)
    env.step = step_spy
    env.reset()
    env.step = orig_step
    assert len(LOG) == 3 and tuple(LOG[0].shape) == (n, 4) and tuple(LOG[1].shape) == (n,), [tuple(d.shape) for d in LOG]
    draw_reset[:, 0:4] = LOG[0].numpy()
    draw_reset[:, 4] = LOG[1].numpy()
    mask = LOG[1].numpy() > np.float32(CFG["zero_rom_dist_llh"])
    assert tuple(LOG[2].shape) == (int(mask.sum()), 2)
    draw_reset[mask, 5:7] = LOG[2].numpy()
    del LOG[:]
    obs = env.get_observations()
    snap(obs, torch.zeros(n, 2), state["k0"], state["n0"])
    x[:, 0], pz_x[:, 0], z[:, 0] = env.get_state(), env.rom.proj_z(env.root_states.clone()), tg.trajectory[:, 0, :]
    for t in range(T):
        k = tg.k.clone()
        while torch.any(tg.k == k):
            kb, nb = tg.k.numpy().copy(), np.array([len(r) for r in resamples], np.int32)
            actions = policy(obs.detach())
            obs, _, _, dones, _ = env.step(actions.detach())
            snap(obs, actions, kb, nb)
        proj = env.rom.proj_z(env.root_states.clone())
        done[:, t] = dones
        v[:, t], x[:, t + 1], z[:, t + 1], pz_x[:, t + 1] = tg.v, env.get_state(), tg.get_trajectory()[:, 0, :], proj
    assert not LOG, "draws outside a resample after the reset"

    R = max(len(r) for r in resamples)
    draw_resample = np.zeros((n, R, 20), np.float32)
    for e, r in enumerate(resamples):
        draw_resample[e, :len(r)] = np.stack(r)
    nres = np.array([len(r) for r in resamples], np.int32)
    # conditions the tests rely on
    assert nres.min() >= 3, "every env resamples at least twice after the reset's own"
    assert in_reset_loop.any(), "no env resamples inside the reset loop"
    assert np.stack([s["stationary"] for s in steps]).any(), "no env is ever stationary"
    assert (~mask).any() and mask.any(), "start offsets: need both zero and non-zero"
    assert all(s["stepped"].all() or not s["stepped"].any() for s in steps), "the clock is common to all envs"

    out = {"meta_cfg": np.array(json.dumps(CFG)), "meta_T": np.array(T), "draw_reset": draw_reset, "draw_resample": draw_resample,
           "n_resample": nres, "offset_mask": mask, "in_reset_loop": in_reset_loop,
           "z": z.numpy(), "v": v.numpy(), "pz_x": pz_x.numpy(), "done": done.numpy(), "x": x.numpy()}
    for key in ("k", "t", "t_final", "stationary", "weights", "extreme", "nres", "stepped", "resampled", "root", "obs", "act", "tg_row",
                "tg_traj", "v_traj", "trajectory"):
        out["st_" + key] = np.stack([s[key] for s in steps])
    dst = os.path.join(ROOT, "tests", "golden", "rom_sim_double_single.npz")
    np.savez_compressed(dst, **out)
    print(f"{dst}: {len(steps)} env steps, R = {R}, resamples per env {nres.min()}..{nres.max()}, in the reset loop "
          f"{int(in_reset_loop.sum())} envs, zero offset {int((~mask).sum())} envs, {os.path.getsize(dst) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
