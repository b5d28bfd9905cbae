"""The closed-form row rule of the device dataset builder (csrc/tube_data_kernels.hip) as plain loops over
(env, step, block, column), in float32 with one rounding per operation.  It restates tube/data.py, which is pinned to the reference by
tests/golden/tube_rows.npz; tests/test_tube_device_data_host.py checks the two against each other and against that fixture."""
import numpy as np

f32 = np.float32


def norm32(pz, z):
    """|pz - z|: the squares summed in column order, then the square root; every operation rounded to float32."""
    s = f32(0)
    for k in range(len(z)):
        d = f32(pz[k]) - f32(z[k])
        s = f32(s + f32(d * d))
    return np.sqrt(s, dtype=f32)


def lead(kind, z, pz):
    """The leading (error) quantity of one record sample."""
    if kind == "scalar":
        return [norm32(pz, z)]
    d = [f32(pz[k]) - f32(z[k]) for k in range(len(z))]
    return [f32(abs(x)) for x in d] if kind == "vector" else d


def base_row(kind, recursive, z, pz, v, zero_v=False):
    vv = [f32(0)] * len(v) if zero_v else list(v)
    if kind == "scalar":
        return ([norm32(pz, z)] if recursive else []) + list(z[2:]) + vv
    return lead(kind, z, pz) + list(z) + vv


def dims(kind, N, recursive, n, m):
    if kind == "scalar":
        return (N * (1 + n - 2 + m) if recursive else 1 + N * (n - 2 + m)), 1
    return N * (2 * n + m), n


def sequences(kind, z, pz_x, v, N=1, dN=1, recursive=False):
    """data (E, T, input_dim), target (E, T, output_dim): every row, in (env, time) order."""
    E, T = v.shape[:2]
    I, O = dims(kind, N, recursive, z.shape[2], v.shape[2])
    data, target = np.zeros((E, T, I), f32), np.zeros((E, T, O), f32)
    for e in range(E):
        for t in range(T):
            row = [norm32(pz_x[e, t], z[e, t])] if kind == "scalar" and not recursive else []
            for i in range(N):
                src = (T - 1 - i * dN) - (T - 1 - t) * dN
                s = max(src, 0)
                row += base_row(kind, recursive, z[e, s], pz_x[e, s], v[e, s], zero_v=src < 0)
            data[e, t] = row
            target[e, t] = lead(kind, z[e, t + 1], pz_x[e, t + 1])
    return data, target


def keep_mask(done, mark_last_env=False, epoch_envs=None):
    keep = np.logical_not(np.asarray(done, bool))
    if mark_last_env:
        k = keep.shape[0] if epoch_envs is None else epoch_envs
        keep[np.arange(keep.shape[0]) % k == k - 1] = False
    return keep


def rows(kind, rec, N=1, dN=1, recursive=False, mark_last_env=False, epoch_envs=None):
    """The compacted rows: sequences() without the done steps, in (env, time) order."""
    data, target = sequences(kind, rec["z"], rec["pz_x"], rec["v"], N, dN, recursive)
    keep = keep_mask(rec["done"], mark_last_env, epoch_envs).reshape(-1)
    return data.reshape(keep.size, -1)[keep], target.reshape(keep.size, -1)[keep]


def horizon(rec, H_rev):
    """ScalarHorizonTubeDataset.from_folder's w, z without its position, v: padded in front by H_rev steps."""
    z, pz, v = rec["z"], rec["pz_x"], rec["v"]
    E, T, m = v.shape
    w, zn, vp = np.zeros((E, T + H_rev), f32), np.zeros((E, T + H_rev, z.shape[2] - 2), f32), np.zeros((E, T + H_rev, m), f32)
    for e in range(E):
        for tp in range(T + H_rev):
            s = max(tp - H_rev, 0)
            w[e, tp] = norm32(pz[e, s], z[e, s])
            zn[e, tp] = z[e, s, 2:]
            if tp >= H_rev:
                vp[e, tp] = v[e, s]
    return w, zn, vp
