"""Our own numpy restatement of the command tracker (include/legged_hip.h lg_cmdtrack_*; the reference's
deep_tube_learning/data_collection_velocity.py:112-156 with SingleInt2D.des_pose_vel, quat2yaw, yaw2rot, wrap_angles), in float64
(the yardstick) or float32 (one numpy float32 operation per device operation, in the device's order).

The generator is tests/rom_sim_ref.py's RomSimRef.resample / input as they are, fed the same recorded draws as the device
(``reset`` (N, 9), of which only the construction's ramp_v_end, slots 7:9, is read; ``resample`` (N, R, 20)); its clock is float32
in both modes.  Constants enter as their float32 values, as the device holds them -- except pi, which is the float32 pi in float32
and numpy's in float64 (wrap_angles itself).
"""
import numpy as np

from tests.rom_sim_ref import RomSimRef

F = np.float32
RANDOM, PLAN = 0, 4


def quat2yaw(q, D):
    """The xyz-Euler yaw of scipy's Rotation.from_quat(q).as_euler('xyz')[:, 2] for q = xyzw of any norm:
    atan2(R10, R00) |q|^2 = atan2(2 (xy + wz), w^2 + x^2 - y^2 - z^2)."""
    x, y, z, w = (q[:, k].astype(D) for k in range(4))
    return np.arctan2(D(2) * (x * y + w * z), ((w * w + x * x) - y * y) - z * z)


def wrap(a, D):
    """((a + pi) mod 2 pi) - pi, mod in Python's floor sense."""
    pi = D(np.pi) if D is np.float64 else F(np.pi)
    two_pi = D(2) * pi
    return np.mod(a + pi, two_pi) - pi


def command(cfg, z, v, root, D, parts=None):
    """u (N, 3) before the observation scale, for ROM state z, input v (N, 2) and root_states (N, 13).  parts: a dict that
    receives the raw (unclipped) command and the wrap argument, for the tests' margins."""
    c32 = lambda name: np.asarray(cfg[name], F).astype(D)
    z, v = z.astype(D), v.astype(D)
    yaw = quat2yaw(root[:, 3:7], D)
    c, s = np.cos(yaw), np.sin(yaw)
    e0, e1 = z[:, 0] - root[:, 0].astype(D), z[:, 1] - root[:, 1].astype(D)
    arg = np.arctan2(v[:, 1], v[:, 0]) - yaw
    e2 = wrap(arg, D) if cfg["track_yaw"] else np.zeros_like(e0)
    el = [c * e0 + s * e1, (-s) * e0 + c * e1, e2]
    vl = [c * v[:, 0] + s * v[:, 1], (-s) * v[:, 0] + c * v[:, 1], np.zeros_like(e0)]
    Kp, lo, hi = c32("Kp"), c32("u_min"), c32("u_max")
    raw = np.stack([vl[j] + ((Kp[3 * j] * el[0] + Kp[3 * j + 1] * el[1]) + Kp[3 * j + 2] * el[2]) for j in range(3)], 1)
    if parts is not None:
        parts["raw"], parts["wrap_arg"] = raw, arg
    return np.minimum(np.maximum(raw, lo), hi).astype(D)


class CmdTrackRef:
    """begin(root) / step(t, root, done) as lg_cmdtrack_begin / lg_cmdtrack_step; records env-major in self.rec, the command
    written to the observation after each call in self.cmd (a list of (N, 3), scale applied), the margins of each in self.parts."""

    def __init__(self, cfg, n, T, dtype=np.float64, draws_reset=None, draws_resample=None, plan=None):
        self.c, self.n, self.T, self.D = cfg, n, T, np.dtype(dtype).type
        D = self.D
        self.plan = None if plan is None else np.asarray(plan, F)
        self.gen = None
        if cfg["kind"] == RANDOM:
            self.gen = RomSimRef(cfg, draws_reset, draws_resample, dtype)
        self.rec = {"z": np.zeros((n, T + 1, 2), D), "v": np.zeros((n, T, 2), D), "pz_x": np.zeros((n, T + 1, 2), D),
                    "done": np.zeros((n, T), bool), "u": np.zeros((n, T, 3), D)}
        self.cmd, self.parts, self.nres, self.resampled = [], [], [], []

    def _gen_reset(self):
        """TrajectoryGenerator.reset without its window: RomSimRef.reset's generator lines."""
        g, c = self.gen, self.c
        if not g.constructed:
            g.ramp_v1 = g._uni(g._c("rom_v_min"), g._c("rom_v_max"), g.dr[:, 7:9])
            g.constructed = True
        g.k[:] = F(-g.N)
        g.t = g.k * F(c["rom_dt"])
        g.t_final = g.k * F(c["rom_dt"])
        g.nres[:] = 0
        g.resample(np.arange(self.n))
        for _ in range(g.N):
            g.v = g.input(g.t)
            g.t = g.t + F(c["rom_dt"])

    def _input(self, t):
        if self.gen is not None:
            v = self.gen.input(np.full(self.n, F(t), F) * F(self.c["rom_dt"]))
            self.nres.append(self.gen.nres.copy())
            self.resampled.append(self.gen.resampled.copy())
            return v
        v = np.zeros((self.n, 2), self.D)
        if self.plan is not None and t < self.plan.shape[1]:
            v = self.plan[:, t].astype(self.D)
        return v

    def _command(self, t, root):
        D = self.D
        self.v = self._input(t)
        parts = {}
        self.u = command(self.c, self.z, self.v, root, D, parts)
        self.parts.append(parts)
        self.cmd.append(self.u * np.asarray(self.c["cmd_scale"], F).astype(D))

    def begin(self, root):
        root = np.asarray(root, F)
        if self.gen is not None:
            self._gen_reset()
        self.z = root[:, :2].astype(self.D)
        self.rec["z"][:, 0], self.rec["pz_x"][:, 0] = self.z, self.z
        if self.T > 0:
            self._command(0, root)

    def step(self, t, root, done):
        root, done, D = np.asarray(root, F), np.asarray(done).astype(bool), self.D
        r = self.rec
        r["done"][:, t], r["v"][:, t], r["u"][:, t] = done, self.v, self.u
        z = self.z + np.asarray(self.c["rom_dt"], F).astype(D) * self.v
        z[done] = root[done, :2].astype(D)
        r["z"][:, t + 1], r["pz_x"][:, t + 1] = z, root[:, :2].astype(D)
        self.z = z
        if t + 1 < self.T:
            self._command(t + 1, root)
