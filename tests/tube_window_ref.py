"""Test-only restatements of the windowed closed-loop roll-out, in torch at any dtype.

rollout_rule      the rule HipTubeModel.rollout_window implements, for any model callable on a batch of rows
shift_register    the loop of deep_tube_learning/evaluation/evaluate_tube_simple.py:62-72 (recursive scalar window, dN = 1)
gather            the loop of evaluate_error_dyn_simple.py:44-50, with the dataset's front padding where the reference indexes
                  fe[t - n*dN] with a negative index (Python wraps those to the end of the array)
delayed_window    the window those two scripts assume: block i is the row delayed by exactly i * dN steps, the front filled
                  with the first sample whose last m columns are zeroed.  For dN = 1 this is tube.data.sliding_window.
"""
import torch


def rollout_rule(f, x, fb, taps, dN, stride, reseed=None):
    """out[s, t] = f(xt), xt = x[s, t] except that for every tap i with t - i*dN > s0(t) columns [i*stride, i*stride + fb) are
    out[s, t-1-i*dN, :fb]; s0(t): the last step <= t that is 0 or has reseed[s, t] set.  f maps (n, I) rows to (n, O)."""
    n, T, _ = x.shape
    out, age = [], torch.zeros(n, dtype=torch.long, device=x.device)
    for t in range(T):
        xt = x[:, t].clone()
        if t > 0:
            age = age + 1 if reseed is None else torch.where(reseed[:, t].bool(), torch.zeros_like(age), age + 1)
        for i in range(taps):
            lag = i * dN
            if t - 1 - lag < 0:
                break
            c0 = i * stride
            xt[:, c0:c0 + fb] = torch.where((age > lag)[:, None], out[t - 1 - lag][:, :fb].to(xt.dtype), xt[:, c0:c0 + fb])
        out.append(f(xt))
    return torch.stack(out, 1)


def delayed_window(data, N, dN, m):
    """data (T, c) -> (T, N * c): block i of row t is data[t - i*dN], or data[0] with its last m columns zeroed where
    t - i*dN < 0."""
    T = data.shape[0]
    first = data[0].clone()
    first[-m:] = 0
    blocks = []
    for i in range(N):
        k = min(i * dN, T)
        blocks.append(torch.cat((first[None].repeat(k, 1), data[:T - k]), 0))
    return torch.cat(blocks, 1)


def shift_register(f, single_data, rep_dim):
    """evaluate_tube_simple.py:62-72, recursive branch, for one sequence.  single_data (T, N * rep_dim): the windowed rows, column
    0 of every block the error norm w.  Returns (T, 1): entry t is the script's fw[t + 1] (the script stops one step earlier)."""
    T = single_data.shape[0]
    out = []
    data = single_data[0].clone()
    for t in range(T):
        fw_next = f(data[None])[0]
        out.append(fw_next)
        if t + 1 < T:
            data[rep_dim:] = data[:-rep_dim].clone()
            data[0] = fw_next[0]
            data[1:rep_dim] = single_data[t + 1, 1:rep_dim]
    return torch.stack(out, 0)


def gather(f, e, z, v, N, dN):
    """evaluate_error_dyn_simple.py:44-50 for one sequence: e (T, n) the signed error, z (T, n), v (T, m).  Block k of the input
    at step t is (fe[t - k*dN], z[t - k*dN], v[t - k*dN]) with fe[0] = e[0] and fe[t + 1] the model's output at step t; where
    t - k*dN < 0 the block is the dataset's padding (e[0], z[0], 0).  Returns (T, n): entry t is the script's fe[t + 1]."""
    T = e.shape[0]
    fe = e.clone()
    pad = torch.cat((e[0], z[0], torch.zeros_like(v[0])))
    out = []
    for t in range(T):
        blocks = []
        for k in range(N):
            s = t - k * dN
            blocks.append(torch.cat((fe[s], z[s], v[s])) if s >= 0 else pad)
        y = f(torch.cat(blocks)[None])[0]
        out.append(y)
        if t + 1 < T:
            fe[t + 1] = y
    return torch.stack(out, 0)
