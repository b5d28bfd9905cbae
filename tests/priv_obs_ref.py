"""float32 numpy restatement of the privileged observation row (include/legged_hip.h lg_priv_obs_*, csrc/privobs_kernels.hip) from
the env's own buffers: one fp32 operation per line, in the kernel's order, so the comparison is bit for bit.

``t``: name -> numpy array of the env buffers (HipEnvCore.t, copied to the host after the step); ``cs``: the env's lg_cfg struct
(HipEnvCore.cfg_struct); ``spec``: envs/base/privileged_obs.PrivilegedObsSpec."""
import numpy as np

f32 = np.float32


def obs_before_noise(t, cs):
    """The policy observation before noise and before the clip (legged_robot.py:208-226 / legged_robot_trajectory.py:280-288)."""
    N, A, O = t["root_states"].shape[0], int(cs.num_actions), int(cs.num_obs)
    out = np.zeros((N, O), f32)
    out[:, 0:3] = t["base_lin_vel"] * f32(cs.obs_scale_lin_vel)
    out[:, 3:6] = t["base_ang_vel"] * f32(cs.obs_scale_ang_vel)
    out[:, 6:9] = t["projected_gravity"] * f32(1.0)
    if cs.traj.enabled:
        Nt = int(cs.traj.N)
        d = t["trajectory"].reshape(N, Nt, 2) - t["root_states"][:, None, 0:2]
        d = d * np.array([cs.traj.obs_scale[0], cs.traj.obs_scale[1]], f32)
        out[:, 9:9 + 2 * Nt] = d.reshape(N, 2 * Nt)
        ob = 9 + 2 * Nt
    else:
        out[:, 9:11] = t["commands"][:, 0:2] * f32(cs.obs_scale_lin_vel)
        out[:, 11] = t["commands"][:, 2] * f32(cs.obs_scale_ang_vel)
        ob = 12
    default = np.array([cs.default_dof_pos[j] for j in range(A)], f32)
    q = t["dof_state"][:, :, 0] - default
    out[:, ob:ob + A] = q * f32(cs.obs_scale_dof_pos)
    out[:, ob + A:ob + 2 * A] = t["dof_state"][:, :, 1] * f32(cs.obs_scale_dof_vel)
    out[:, ob + 2 * A:ob + 3 * A] = t["actions"]
    if cs.measure_heights:
        out[:, ob + 3 * A:] = heights(t, cs)
    assert out.dtype == f32
    return out


def heights(t, cs):
    H = int(cs.num_height_points)
    h = t["root_states"][:, 2:3] - f32(0.5)
    h = h - t["measured_heights"][:, :H]
    h = np.minimum(np.maximum(h, f32(-1.0)), f32(1.0))
    return h * f32(cs.obs_scale_height)


def body_contact(t, cs):
    """(flags, float64 squared norms) of the penalised bodies: fx fx + fy fy + fz fz > 0.01, each product and sum rounded."""
    pen = [int(cs.pen_idx[b]) for b in range(int(cs.num_pen))]
    f = t["contact_forces"][:, pen, :]
    n2 = f[..., 0] * f[..., 0]
    n2 = n2 + f[..., 1] * f[..., 1]
    n2 = n2 + f[..., 2] * f[..., 2]
    return (n2 > f32(0.01)).astype(f32), (f.astype(np.float64) ** 2).sum(-1)


def raw_term(name, t, cs):
    N = t["root_states"].shape[0]
    feet = [int(cs.feet_idx[k]) for k in range(int(cs.num_feet))]
    if name == "obs":
        return obs_before_noise(t, cs)
    if name == "friction":
        return t["friction"].reshape(N, 1)
    if name == "base_mass":
        return t["base_mass_delta"].reshape(N, 1)
    if name == "material":
        return t["material"].reshape(N, 4)
    if name == "feet_contact_forces":
        return t["contact_forces"][:, feet, :].reshape(N, 3 * len(feet))
    if name == "feet_contact":
        return (t["contact_forces"][:, feet, 2] > f32(1.0)).astype(f32)
    if name == "feet_air_time":
        return t["feet_air_time"].reshape(N, len(feet))
    if name == "body_contact":
        return body_contact(t, cs)[0]
    if name == "torques":
        return t["torques"]
    if name == "heights":
        return heights(t, cs)
    if name == "episode_progress":
        inv_max_len = f32(1.0 / float(cs.max_episode_length))
        return (t["episode_length"].astype(f32) * inv_max_len).reshape(N, 1)
    raise KeyError(name)


def restate(t, cs, spec):
    """The (N, W) row and, per term, the unclipped raw * scale block (to see which entries the clip moved)."""
    clip = f32(cs.clip_obs)
    blocks, scaled = [], {}
    for name, scale in zip(spec.terms, spec.scales):
        raw = np.ascontiguousarray(raw_term(name, t, cs), f32)
        v = raw * f32(scale)
        scaled[name] = v
        blocks.append(np.minimum(np.maximum(v, -clip), clip))
    row = np.concatenate(blocks, axis=1)
    assert row.dtype == f32 and row.shape[1] == spec.width
    return row, scaled
