"""Test-only restatement of the one-step tube rolled along a plan (tube_kind 'nn_step'), in torch at any
dtype: the taps, the row of a node, the roll w[k+1] = fw(row_k) and the calibration-to-offset mapping.

Inputs as lg_plan_score takes them: e (B, H_rev) holds w_{-H_rev} .. w_{-1}, v_prev (B, H_rev, 2), w0 (B), v (B, N, 2).
    vv(j) = v[j] for j >= 0, v_prev[H_rev + j] for j < 0
    ww(j) = fw[j-1] for j >= 1, w0 for j = 0, e[H_rev + j] for j < 0
    row_k = [ww(k), vv(k), vv(k-1), .., vv(k-T+1), (level)]                       not recursive, I' = 1 + 2 T
    row_k = [ww(k), vv(k), ww(k-1), vv(k-1), .., ww(k-T+1), vv(k-T+1), (level)]   recursive,     I' = 3 T
    fw[k] = MLP(row_k): the raw value is fed back, never the calibrated one.
"""
import torch


def taps(input_dim, level, recursive):
    """T from the width of the row; None where the width fits the layout in no T >= 1."""
    Ip = input_dim - int(bool(level))
    if Ip < 3:
        return None
    if recursive:
        return Ip // 3 if Ip % 3 == 0 else None
    return (Ip - 1) // 2 if (Ip - 1) % 2 == 0 else None


def _history(e, v_prev, w0, v, fw):
    """ww (B, H_rev + N) and vv (B, H_rev + N, 2) over steps -H_rev .. N-1; fw None: zeros where the model's own output goes."""
    B, N = v.shape[:2]
    tail = torch.zeros(B, N - 1, dtype=v.dtype) if fw is None else fw[:, :N - 1].to(v.dtype)
    return torch.cat([e, w0[:, None], tail], dim=1), torch.cat([v_prev, v], dim=1)


def rows(e, v_prev, w0, v, T, recursive, level=None, fw=None):
    """x (B, N, I): the row of every node.  fw (B, >= N - 1): the values fed back; None leaves those columns 0 -- the teacher rows a
    closed-loop roll-out (rollout / rollout_window, no reseed) overwrites with its own output."""
    B, N = v.shape[:2]
    Hr = e.shape[1]
    assert Hr >= T - 1, "the delayed taps of node 0 come from the caller's history"
    ww, vv = _history(e, v_prev, w0, v, fw)
    out = []
    for k in range(N):
        cols = []
        for i in range(T):
            j = Hr + k - i
            if recursive or i == 0:
                cols.append(ww[:, j, None])
            cols.append(vv[:, j])
        if level is not None:
            cols.append(torch.full((B, 1), float(level), dtype=v.dtype))
        out.append(torch.cat(cols, dim=1))
    return torch.stack(out, dim=1)


def roll(f, e, v_prev, w0, v, T, recursive, level=None):
    """fw (B, N) by the literal loop: node k's row from the values made so far, fw[k] = f(row_k)[:, 0].  f maps (B, I) to (B, 1)."""
    B, N = v.shape[:2]
    fw = torch.zeros(B, N, dtype=v.dtype)
    for k in range(N):
        fw[:, k] = f(rows(e, v_prev, w0, v[:, :k + 1], T, recursive, level, fw)[:, k])[:, 0]
    return fw


def offsets(calibration, N, coverage=None, level=None, trajectory=False):
    """(N) offsets added to fw[0..N-1].  A per-age calibration (it has max_age): fw[k] is k fed-back steps after the seed, so
    offset[k] = offsets[coverage, min(k, max_age - 1)] (+ the margin with trajectory).  A flat / levels one: its one_step offset
    at k = 0, its rollout offset at k >= 1."""
    if hasattr(calibration, "max_age"):
        c = calibration.index(coverage)
        off = torch.stack([calibration.offsets[c, min(k, calibration.max_age - 1), 0] for k in range(N)])
        return off + calibration.margin[c, 0] if trajectory else off
    c = calibration.index(coverage, level)
    return torch.stack([calibration.offsets[0 if k == 0 else 1, c, 0] for k in range(N)])
