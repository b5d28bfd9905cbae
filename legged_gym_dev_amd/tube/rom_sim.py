"""HipRomSim: the reference's ROM-on-ROM simulator (deep_tube_learning/custom_sim.py CustomSim with the `custom` branch of
data_collection_trajectory.py:87-90) on the HIP kernels of romsim_kernels.hip (lg_romsim_* in include/legged_hip.h).

A DoubleInt2D "robot" tracks the random trajectory of the SingleInt2D reduced-order model under the DoubleSingleTracking law:
tube data (``epoch_<k>.pickle``) without a trained policy or the articulated-body env.  ``collect_epoch`` runs a whole epoch --
reset, every env step, every record -- in one launch; ``reset`` / ``step`` / ``policy`` give CustomSim's surface, one launch per
call, so that scripts/collect_trajectory_data.py::collect runs on it unchanged (the cross-check of the fused path: both give the
same bits).  There is no CPU fallback: without the library or a GPU the constructor raises.
"""
import ctypes as C
import types

from .. import capi
from ..envs.base.base_config import BaseConfig, S, cfg_class

# configs/data_generation/double_single_int.yaml (with default_custom.yaml), field for field
RomSimCfg = cfg_class("RomSimCfg", BaseConfig, dict(
    env=S(num_envs=8192, episode_length_s=20,
          model=S(cls='DoubleInt2D', dt=0.05, z_min=[-1e9, -1e9, -0.3, -0.3], z_max=[1e9, 1e9, 0.3, 0.3], v_min=[-0.5, -0.5],
                  v_max=[0.5, 0.5])),
    rom=S(cls='SingleInt2D', dt=0.1, z_min=[-1e9, -1e9], z_max=[1e9, 1e9], v_min=[-0.2, -0.2], v_max=[0.2, 0.2]),
    trajectory_generator=S(cls='TrajectoryGenerator', t_samp_cls='UniformSampleHoldDT', weight_samp_cls='UniformWeightSamplerNoRamp',
                           N=10, t_low=1, t_high=2, freq_low=0.01, freq_high=2, prob_stationary=0.0005, dN=1),
    controller=S(cls='DoubleSingleTracking', Kp=10, Kd=10),
    domain_rand=S(randomize_rom_distance=True, max_rom_distance=[1.0, 1.0], zero_rom_dist_llh=0.25),
    init_state=S(default_noise_lower=[0.0, 0.0, -0.1, -0.1], default_noise_upper=[0.0, 0.0, 0.1, 0.1]),
), doc="Configuration of HipRomSim; the defaults are the reference's double_single_int.yaml.", module=__name__)

MAX_N = capi.TRAJ_MAX_PTS - 1


def check_envelope(cfg):
    """The supported envelope (lg_romsim_check_cfg refuses the same); raises ValueError naming the field outside it."""
    tg = cfg.trajectory_generator
    if cfg.env.model.cls != 'DoubleInt2D':
        raise ValueError(f"env.model.cls={cfg.env.model.cls!r}: only 'DoubleInt2D' is supported")
    if cfg.rom.cls != 'SingleInt2D':
        raise ValueError(f"rom.cls={cfg.rom.cls!r}: only 'SingleInt2D' is supported")
    if cfg.controller.cls != 'DoubleSingleTracking':
        raise ValueError(f"controller.cls={cfg.controller.cls!r}: only 'DoubleSingleTracking' is supported")
    if tg.cls != 'TrajectoryGenerator':
        raise ValueError(f"trajectory_generator.cls={tg.cls!r}: only 'TrajectoryGenerator' is supported on this simulator "
                         "(the Zero / Square / Circle generators are not)")
    if tg.t_samp_cls != 'UniformSampleHoldDT':
        raise ValueError(f"trajectory_generator.t_samp_cls={tg.t_samp_cls!r}: only 'UniformSampleHoldDT' is supported")
    if tg.weight_samp_cls not in capi.TG_WEIGHT_SAMPLERS:
        raise ValueError(f"trajectory_generator.weight_samp_cls={tg.weight_samp_cls!r}: one of {tuple(capi.TG_WEIGHT_SAMPLERS)}")
    if tg.dN != 1:
        raise ValueError(f"trajectory_generator.dN={tg.dN}: must be 1")
    if not 2 <= tg.N <= MAX_N:
        raise ValueError(f"trajectory_generator.N={tg.N}: 2..{MAX_N} (N = 1 has no v_trajectory[:, 1])")
    if not 0 < cfg.env.model.dt <= cfg.rom.dt:
        raise ValueError(f"env.model.dt={cfg.env.model.dt}: must satisfy 0 < model.dt <= rom.dt = {cfg.rom.dt}")
    if cfg.env.num_envs < 1:
        raise ValueError(f"env.num_envs={cfg.env.num_envs}: must be positive")
    if not 0 < tg.t_low <= tg.t_high:
        raise ValueError(f"trajectory_generator.t_low={tg.t_low}, t_high={tg.t_high}: must satisfy 0 < t_low <= t_high")
    if int(cfg.env.episode_length_s / cfg.rom.dt) < 1:
        raise ValueError(f"env.episode_length_s={cfg.env.episode_length_s}: T = int(episode_length_s / rom.dt) must be at least 1")


def to_struct(cfg, seed=0, env_offset=0):
    """lg_romsim_cfg of a RomSimCfg; class names outside the envelope become a non-zero selector (refused by the C side)."""
    tg, m = cfg.trajectory_generator, cfg.env.model
    c = capi.lg_romsim_cfg()
    c.num_envs, c.env_offset, c.N, c.dN = int(cfg.env.num_envs), int(env_offset), int(tg.N), int(tg.dN)
    c.model_cls = 0 if m.cls == 'DoubleInt2D' else 1
    c.rom_cls = 0 if cfg.rom.cls == 'SingleInt2D' else 1
    c.controller_cls = 0 if cfg.controller.cls == 'DoubleSingleTracking' else 1
    c.generator_cls = capi.TG_KINDS.get(tg.cls, -1)
    c.t_samp_cls = 0 if tg.t_samp_cls == 'UniformSampleHoldDT' else 1
    c.weight_sampler = capi.TG_WEIGHT_SAMPLERS.get(tg.weight_samp_cls, -1)
    c.randomize_rom_distance = int(bool(cfg.domain_rand.randomize_rom_distance))
    c.seed = int(seed)
    c.model_dt, c.rom_dt, c.Kp, c.Kd = float(m.dt), float(cfg.rom.dt), float(cfg.controller.Kp), float(cfg.controller.Kd)
    c.model_z_min[:], c.model_z_max[:] = [float(v) for v in m.z_min], [float(v) for v in m.z_max]
    c.model_v_min[:], c.model_v_max[:] = [float(v) for v in m.v_min], [float(v) for v in m.v_max]
    c.rom_v_min[:], c.rom_v_max[:] = [float(v) for v in cfg.rom.v_min], [float(v) for v in cfg.rom.v_max]
    c.t_low, c.t_high, c.freq_low, c.freq_high = float(tg.t_low), float(tg.t_high), float(tg.freq_low), float(tg.freq_high)
    c.prob_stationary, c.zero_rom_dist_llh = float(tg.prob_stationary), float(cfg.domain_rand.zero_rom_dist_llh)
    c.max_rom_dist[:] = [float(v) for v in cfg.domain_rand.max_rom_distance]
    c.noise_lo[:] = [float(v) for v in cfg.init_state.default_noise_lower]
    c.noise_hi[:] = [float(v) for v in cfg.init_state.default_noise_upper]
    return c


class HipRomSim:
    """CustomSim's surface on one lg_romsim context; every tensor is a zero-copy view of library-owned HBM."""

    def __init__(self, cfg=None, seed=0, device="cuda:0", env_offset=0):
        import torch
        from ..lib import LeggedHipError, device_tensor, load
        self.cfg = cfg if cfg is not None else RomSimCfg()
        check_envelope(self.cfg)
        self._err = LeggedHipError
        self.lib = load()
        self.device = torch.device(device)
        if self.device.type != "cuda" or not torch.cuda.is_available():
            raise LeggedHipError("the HIP ROM simulator needs a GPU device (no CPU fallback); got " + str(device))
        torch.cuda.set_device(self.device)
        self.num_envs = int(self.cfg.env.num_envs)
        self.max_episode_length_s = self.cfg.env.episode_length_s
        self.dt = self.cfg.env.model.dt
        self.ctx = C.c_void_p()
        st = to_struct(self.cfg, seed, env_offset)
        rc = self.lib.lg_romsim_create(C.byref(st), C.byref(self.ctx))
        if rc != 0:
            raise LeggedHipError(f"lg_romsim_create failed ({rc}): {self.lib.lg_last_error().decode()}")
        self._device_tensor = device_tensor
        self._views()
        tg, n = self.cfg.trajectory_generator, self.num_envs
        self.rom = types.SimpleNamespace(n=2, m=2, dt=self.cfg.rom.dt, proj_z=lambda x: x[..., :2])
        ts = self.t["tg_state"]
        self.traj_gen = types.SimpleNamespace(
            N=tg.N, dN=tg.dN, rom=self.rom, k=ts[:, 6], t=ts[:, 5], t_final=ts[:, 4], v=ts[:, 25:27], weights=ts[:, 0:4],
            trajectory=self.t["tg_traj"], v_trajectory=self.t["v_traj"], get_trajectory=lambda: self.t["trajectory"],
            get_v_trajectory=lambda: self.t["v_traj"])
        self.root_states = self.t["root_states"]
        self.use_current_stream()

    def _views(self):
        b = capi.lg_romsim_buffers()
        self.lib.lg_romsim_get_buffers(self.ctx, C.byref(b))
        n, N = self.num_envs, int(self.cfg.trajectory_generator.N)
        shapes = {"root_states": ((n, 4), "f4"), "tg_state": ((n, capi.TG_STRIDE), "f4"), "tg_traj": ((n, N + 1, 2), "f4"),
                  "v_traj": ((n, N, 2), "f4"), "trajectory": ((n, N, 2), "f4"), "obs": ((n, capi.RS_NOBS), "f4"),
                  "actions": ((n, 2), "f4"), "done": ((n,), "u1"), "n_resample": ((n,), "i4"), "inject_overrun": ((1,), "i4")}
        if b.inject_K:
            shapes["inject"] = ((n, int(b.inject_K)), "f4")
        self.t = getattr(self, "t", {})
        for name, (shape, dt) in shapes.items():
            ptr = C.cast(getattr(b, name), C.c_void_p).value
            if name not in self.t or self.t[name].data_ptr() != ptr or tuple(self.t[name].shape) != shape:
                self.t[name] = self._device_tensor(ptr, shape, dt, self, self.device)

    def use_current_stream(self):
        import torch
        self.lib.lg_romsim_set_stream(self.ctx, C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))

    def call(self, fn, *args):
        rc = getattr(self.lib, "lg_romsim_" + fn)(self.ctx, *args)
        if rc != 0:
            raise self._err(f"lg_romsim_{fn} failed ({rc}): {self.lib.lg_last_error().decode()}")

    # ---- CustomSim's surface
    def reset(self):
        """CustomSim.reset (custom_sim.py:77-78).  Returns (observation, None), what collect() unpacks."""
        self.call("reset", None, self.num_envs)
        return self.t["obs"], None

    def reset_idx(self, env_ids):
        """All envs or nothing: a partial reset is refused (by the C side, with the reason)."""
        self.call("reset", C.c_void_p(env_ids.data_ptr()) if env_ids is not None else None, int(len(env_ids)))

    def step(self, actions):
        """CustomSim.step (custom_sim.py:71-75): actions (N, 2) on the device, or None for the built-in controller."""
        if actions is not None:
            import torch
            actions = actions.to(device=self.device, dtype=torch.float32).contiguous()
            if tuple(actions.shape) != (self.num_envs, 2):
                raise ValueError(f"actions must be ({self.num_envs}, 2), got {tuple(actions.shape)}")
        self.call("step", C.c_void_p(actions.data_ptr()) if actions is not None else None)
        return self.t["obs"], None, None, self.t["done"].view(dtype=self._bool()), None

    def _bool(self):
        import torch
        return torch.bool

    def get_observations(self):
        return self.t["obs"]

    def get_state(self):
        return self.t["root_states"].clone()

    def policy(self, obs):
        """DoubleSingleTracking with DoubleInt2D.clip_v_z (controllers.py:87-92), on the device."""
        import torch
        obs = obs.to(device=self.device, dtype=torch.float32).contiguous()
        out = torch.empty((obs.shape[0], 2), device=self.device, dtype=torch.float32)
        self.call("policy", C.c_void_p(obs.data_ptr()), C.c_void_p(out.data_ptr()), int(obs.shape[0]))
        return out

    def collect_epoch(self, T=None, debug=False):
        """One epoch in one launch: {'z' (N, T+1, 2), 'v' (N, T, 2), 'pz_x' (N, T+1, 2), 'done' (N, T) bool [, 'x' (N, T+1, 4)]},
        device tensors.  T defaults to int(episode_length_s / rom.dt), as the reference's loop."""
        import torch
        if T is None:
            T = int(self.max_episode_length_s / self.rom.dt)
        T, n, f = int(T), self.num_envs, dict(device=self.device, dtype=torch.float32)
        if T < 1:
            self.call("collect", T, None, None, None, None, None)      # refused by the C side, with the reason
        z, pz = torch.empty((n, T + 1, 2), **f), torch.empty((n, T + 1, 2), **f)
        v, done = torch.empty((n, T, 2), **f), torch.empty((n, T), device=self.device, dtype=torch.uint8)
        x = torch.empty((n, T + 1, 4), **f) if debug else None
        self.call("collect", T, C.c_void_p(z.data_ptr()), C.c_void_p(v.data_ptr()), C.c_void_p(pz.data_ptr()),
                  C.c_void_p(done.data_ptr()), C.c_void_p(x.data_ptr()) if debug else None)
        rec = {"z": z, "v": v, "pz_x": pz, "done": done.view(dtype=torch.bool)}
        if debug:
            rec["x"] = x
        return rec

    # ---- replay of recorded draws (tests)
    def inject(self, enable, R=1, constructed=False):
        self.call("inject", int(bool(enable)), int(R), int(bool(constructed)))
        self._views()

    def inject_status(self):
        self.call("inject_status")

    def close(self):
        if getattr(self, "ctx", None):
            self.t = {}
            self.lib.lg_romsim_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
