"""Float64 reference and derived bounds for the rollout's bookkeeping after the policy step: process_env_step (time-out bootstrap, episode
statistics; process_step_body of csrc/ppo_device.h), the GAE scan with its advantage moments (k_gae) and the normalisation
(k_adv_normalize).  Plain loops over the steps on numpy float64 arrays; nothing here comes from the library or from oracle/ppo_torch.py.
tests/test_ppo_rollout_host.py shows that a numpy-float32 emulation of the kernels' order of operations sits inside the bounds;
tests/test_hip_ppo_returns.py runs the cases on the GPU.

Bounds (u = 2^-24; gamma and lambda are the learner's fp32 values, taken exactly):
  bootstrap   r' = fl(r + fl(gamma v)) on a time-out: |r' - ref| <= u (|gamma v| + |r'|);  exact otherwise.
  advantages  per step the scan makes at most 8 roundings (nnt gamma, . next_v, r + ., . - v;  nnt gamma, . lambda, . adv, delta + .), each
              of a value no larger than m_t = |r'_t| + gamma |v_(t+1)| + |v_t| + gamma lambda |A_(t+1)|, and carries the step after it
              with factor gamma lambda:  E_t = 8 u m_t + E_r,t + nnt gamma lambda E_(t+1).
              returns = fl(A + v): E_t + u |ret|;  stored advantage = fl(ret - v): one more rounding, u |a|.
  moments     of the kernel's own stored advantages a (n = N T of them), S1 = sum a, S2 = sum a^2: per-env sequential over T, a 256-wide
              tree (8 levels), one atomic per block in any order: k = T + 8 + ceil(N / 256) roundings on each moment,
              e1 = k u sum |a|,  e2 = (k + 1) u sum a^2 (the square's own rounding).  mean: e1 / n + u |mean|.  The one-pass variance
              (S2 - n mean^2) / (n - 1) subtracts two numbers of size sum a^2 = (n - 1) var + n mean^2: relative to var its error is
              about (k + 5) u (1 + mean^2 / var) -- that factor, not a flat tolerance, is what moment_bounds() propagates.
  normalised  fl((a - mean) inv), inv = fl(1 / (std + 1e-8)): (e_mean + u |a - mean|) inv + |a - mean| e_inv + u |out|.
"""
import numpy as np

U = 2.0 ** -24
f32 = np.float32


def returns64(rew, dones, tos, values, last_v, gamma, lam):
    """rew, values [T][N] fp32, dones / tos [T][N] uint8 (tos None: no time-out bootstrap), last_v [N] fp32.  Returns float64 rewards
    (bootstrap included), returns, raw advantages -- and the bounds E_r, E_ret, E_a of the module docstring."""
    g, l = float(f32(gamma)), float(f32(lam))
    T, N = rew.shape
    r = rew.astype(np.float64)
    v = values.astype(np.float64)
    E_r = np.zeros((T, N))
    if tos is not None:
        boot = g * v * (tos != 0)
        r = r + boot
        E_r = U * (np.abs(boot) + np.abs(r)) * (tos != 0)
    ret, adv_s = np.zeros((T, N)), np.zeros((T, N))
    E_ret, E_a = np.zeros((T, N)), np.zeros((T, N))
    adv, E, next_v = np.zeros(N), np.zeros(N), last_v.astype(np.float64)
    for t in range(T - 1, -1, -1):
        nnt = 1.0 - (dones[t] != 0)
        m = np.abs(r[t]) + g * np.abs(next_v) + np.abs(v[t]) + g * l * np.abs(adv)
        adv = r[t] + nnt * g * next_v - v[t] + nnt * g * l * adv
        E = 8 * U * m + E_r[t] + nnt * g * l * E
        ret[t] = adv + v[t]
        adv_s[t] = adv
        E_ret[t] = E + U * np.abs(ret[t])
        E_a[t] = E_ret[t] + U * np.abs(adv)
        next_v = v[t]
    return dict(rewards=r, returns=ret, adv=adv_s, E_r=E_r, E_ret=E_ret, E_a=E_a)


def moments64(a, N, T):
    """mean, std (unbiased; n - 1 floored at 1 as the kernel does) of the fp32 advantages a, in float64, with their bounds."""
    a = a.astype(np.float64).reshape(-1)
    n = a.size
    k = T + 8 + -(-N // 256)
    S1, S2, Sabs = a.sum(), (a * a).sum(), np.abs(a).sum()
    mean = S1 / n
    den = max(n - 1, 1)
    var = max((S2 - n * mean * mean) / den, 0.0)
    e_mean = k * U * Sabs / n + U * abs(mean)
    e2 = (k + 1) * U * S2
    e_var = (e2 + n * (2 * abs(mean) * e_mean + e_mean * e_mean) + 3 * U * n * mean * mean + U * S2) / den + U * var
    std = np.sqrt(var)
    e_std = max(np.sqrt(var + e_var) - std, std - np.sqrt(max(var - e_var, 0.0))) + U * std
    return dict(mean=mean, std=std, var=var, e_mean=e_mean, e_var=e_var, e_std=e_std, n=n, k=k,
                factor=1 + mean * mean / var if var > 0 else float("inf"))


def normalised64(a, mo):
    """(a - mean) / (std + 1e-8) of the fp32 advantages in float64, and the bound of the docstring."""
    a = a.astype(np.float64)
    eps = float(f32(1e-8))
    inv = 1.0 / (mo["std"] + eps)
    inv_max = 1.0 / (max(mo["std"] - mo["e_std"], 0.0) + eps)
    e_inv = (inv_max - inv) + 2 * U * inv_max
    out = (a - mo["mean"]) * inv
    bound = (mo["e_mean"] + U * np.abs(a - mo["mean"])) * inv_max + np.abs(a - mo["mean"]) * e_inv + U * np.abs(out)
    return out, bound


# ------------------------------------------------------------------------------------------------ the kernels' order in numpy float32
def emulate32(rew, dones, tos, values, last_v, gamma, lam, block_order=None):
    """process_step_body's bootstrap, k_gae and k_adv_normalize operation by operation in numpy float32: per-env sequential scan and sums,
    a 256-wide tree per block, then the blocks' partial sums added in `block_order` (the atomics' order is not fixed)."""
    g, l = f32(gamma), f32(lam)
    T, N = rew.shape
    r = rew.copy()
    if tos is not None:
        r = (rew + g * (values * (tos != 0).astype(f32))).astype(f32)
    ret, a_s = np.zeros((T, N), f32), np.zeros((T, N), f32)
    adv, next_v = np.zeros(N, f32), last_v.astype(f32)
    s1, s2 = np.zeros(N, f32), np.zeros(N, f32)
    for t in range(T - 1, -1, -1):
        nnt = f32(1.0) - (dones[t] != 0).astype(f32)
        delta = r[t] + nnt * g * next_v - values[t]
        adv = (delta + nnt * g * l * adv).astype(f32)
        ret[t] = adv + values[t]
        a = (ret[t] - values[t]).astype(f32)
        a_s[t] = a
        s1 = (s1 + a).astype(f32)
        s2 = (s2 + a * a).astype(f32)
        next_v = values[t]
    nb = -(-N // 256)
    p1, p2 = np.zeros(nb * 256, f32), np.zeros(nb * 256, f32)
    p1[:N], p2[:N] = s1, s2
    p1, p2 = p1.reshape(nb, 256), p2.reshape(nb, 256)
    w = 128
    while w > 0:
        p1[:, :w] += p1[:, w:2 * w]
        p2[:, :w] += p2[:, w:2 * w]
        w >>= 1
    S1 = S2 = f32(0.0)
    for b in (block_order if block_order is not None else range(nb)):
        S1, S2 = f32(S1 + p1[b, 0]), f32(S2 + p2[b, 0])
    cnt = f32(N * T)
    mean = f32(S1 / cnt)
    var = f32(max(f32(f32(S2 - cnt * mean * mean) / f32(max(cnt - f32(1.0), f32(1.0)))), f32(0.0)))
    std = f32(np.sqrt(var))
    inv = f32(f32(1.0) / f32(std + f32(1e-8)))
    return dict(rewards=r, returns=ret, adv=a_s, mean=mean, std=std, norm=((a_s - mean) * inv).astype(f32))


# ------------------------------------------------------------------------------------------------ episode bookkeeping
class Episodes:
    """OnPolicyRunner's cur_reward_sum / cur_episode_length / rewbuffer / lenbuffer as the library keeps them: per-env fp32 running sums
    (one fp32 add per step and env: no order to choose, so the reference is bit-exact), totals over finished episodes, and a ring of the
    last 100.  step() returns what the ring may hold afterwards."""

    def __init__(self, N):
        self.cr, self.cl = np.zeros(N, f32), np.zeros(N, f32)
        self.sum_r, self.sum_abs, self.sum_l, self.count = 0.0, 0.0, 0.0, 0
        self.ring = [None] * 100                      # per slot: (return, length) once it is known

    def step(self, rew, dones):
        """Advances one env step; returns (slots written this step, the (return, length) pairs that finished)."""
        cr, cl = (self.cr + rew).astype(f32), (self.cl + f32(1.0)).astype(f32)
        done = dones != 0
        pairs = sorted(zip(cr[done].tolist(), cl[done].tolist()))
        self.sum_r += float(cr[done].astype(np.float64).sum())
        self.sum_abs += float(np.abs(cr[done]).astype(np.float64).sum())
        self.sum_l += float(cl[done].sum())
        slots = [(self.count + j) % 100 for j in range(len(pairs))]
        self.count += len(pairs)
        self.cr, self.cl = np.where(done, f32(0), cr), np.where(done, f32(0), cl)
        return slots, pairs


# ------------------------------------------------------------------------------------------------ cases
GAMMA, LAM = 0.99, 0.95
# (N, T, time-outs: "on" / "off" (the key present, all zero) / "none" (infos without the key), rewards: mean 0 or mean / std = 3)
CASES = [(N, T, ("on", "off", "none")[(i + j) % 3], ("zero", "three")[(i + j) % 2])
         for i, N in enumerate((1, 255, 256, 257, 300)) for j, T in enumerate((1, 2, 24))] + \
        [(300, 24, "on", "three"), (300, 24, "none", "zero"), (257, 24, "off", "three"), (1, 24, "on", "zero")]
CASES = list(dict.fromkeys(CASES))


def case_id(c):
    return f"N{c[0]}-T{c[1]}-tos-{c[2]}-rew-{c[3]}"


def scenario(N, T, tos_mode, rew_mode, seed=0):
    """Synthetic env outputs: rewards, values (fp32 randn), dones at t = 0 and at t = T - 1 for some envs, one whole step done (the middle
    one), 10 % elsewhere -- with 300 envs over 100 episodes finish in one step and the ring of 100 wraps; time-outs on half the dones.
    last_x [N]: multiples of 2^-10 in [0.5, 6); a critic wired to return x - 3 yields the bootstrap values exactly."""
    g = np.random.default_rng([N, T, seed, len(tos_mode), len(rew_mode)])
    rew = g.standard_normal((T, N)).astype(f32)
    if rew_mode == "three":
        rew = (rew + f32(3.0)).astype(f32)
    values = g.standard_normal((T, N)).astype(f32)
    dones = (g.random((T, N)) < 0.1).astype(np.uint8)
    dones[0, ::3] = 1
    dones[T - 1, int(N > 1)::4] = 1
    dones[T // 2, :] = 1
    tos = None
    if tos_mode == "on":
        tos = ((g.random((T, N)) < 0.5) & (dones != 0)).astype(np.uint8)
        tos[T // 2, ::2] = 1
    elif tos_mode == "off":
        tos = np.zeros((T, N), np.uint8)
    last_x = (g.integers(512, 6144, N) / 1024.0).astype(f32)
    return dict(rew=rew, values=values, dones=dones, tos=tos, last_x=last_x, last_v=(last_x - f32(3.0)).astype(f32))
