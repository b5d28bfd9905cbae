"""On the CPU: a numpy-float32 emulation of the order in which process_step_body, k_gae and k_adv_normalize operate (per-env sequential,
a 256-wide tree, the blocks in any order) sits inside the bounds tests/ppo_rollout_ref.py derives against its float64 loops, and the
scenarios hold what the GPU test says they hold."""
import numpy as np
import pytest

from tests import ppo_rollout_ref as rr


def test_cases_cover_the_sizes_and_regimes():
    assert {c[0] for c in rr.CASES} == {1, 255, 256, 257, 300} and {c[1] for c in rr.CASES} == {1, 2, 24}
    assert {(c[0], c[1]) for c in rr.CASES} == {(N, T) for N in (1, 255, 256, 257, 300) for T in (1, 2, 24)}
    assert {c[2] for c in rr.CASES} == {"on", "off", "none"} and {c[3] for c in rr.CASES} == {"zero", "three"}
    assert any(c[0] == 300 and c[1] == 24 and c[3] == "three" for c in rr.CASES)


@pytest.mark.parametrize("case", rr.CASES, ids=rr.case_id)
def test_fp32_emulation_sits_inside_the_bounds(case):
    N, T, tos_mode, rew_mode = case
    s = rr.scenario(*case)
    assert s["dones"][0].any() and s["dones"][T - 1].any() and s["dones"][T // 2].all()
    assert (s["tos"] is None) == (tos_mode == "none") and (tos_mode != "on" or s["tos"].any()) and (tos_mode != "off" or not s["tos"].any())
    assert np.array_equal((s["last_x"].astype(np.float64) - 3.0).astype(np.float32), s["last_v"])          # x - 3 is exact in fp32
    ref = rr.returns64(s["rew"], s["dones"], s["tos"], s["values"], s["last_v"], rr.GAMMA, rr.LAM)
    nb = -(-N // 256)
    for order in (range(nb), range(nb - 1, -1, -1)):
        em = rr.emulate32(s["rew"], s["dones"], s["tos"], s["values"], s["last_v"], rr.GAMMA, rr.LAM, order)
        assert (np.abs(em["rewards"] - ref["rewards"]) <= ref["E_r"]).all()
        assert (np.abs(em["returns"] - ref["returns"]) <= ref["E_ret"]).all()
        assert (np.abs(em["adv"] - ref["adv"]) <= ref["E_a"]).all()
        mo = rr.moments64(em["adv"], N, T)
        assert abs(float(em["mean"]) - mo["mean"]) <= mo["e_mean"] and abs(float(em["std"]) - mo["std"]) <= mo["e_std"]
        want, bound = rr.normalised64(em["adv"], mo)
        assert (np.abs(em["norm"] - want) <= bound).all()
    if N * T >= 255:
        print(f"{rr.case_id(case)}: mean/std {mo['mean'] / mo['std']:.2f}, 1 + mean^2/var {mo['factor']:.2f}, "
              f"e_std/std {mo['e_std'] / mo['std']:.2e}, advantage bound used {float((np.abs(em['adv'] - ref['adv']) / ref['E_a']).max()):.3f}")
        assert (abs(mo["mean"] / mo["std"]) > 1.0) == (rew_mode == "three")          # the one-pass variance cancels in these, not in those


def test_the_variance_bound_grows_with_the_squared_mean():
    """Same spread, mean 0 against mean 30 std: the bound on the variance follows 1 + mean^2 / var."""
    g = np.random.default_rng(1)
    a = g.standard_normal((24, 300)).astype(np.float32)
    m0, m30 = rr.moments64(a, 300, 24), rr.moments64((a + np.float32(30.0)).astype(np.float32), 300, 24)
    assert m30["factor"] > 800 and m0["factor"] < 1.01
    assert 0.5 * m30["factor"] < (m30["e_var"] / m30["var"]) / (m0["e_var"] / m0["var"]) < 4 * m30["factor"]      # (the mean's own error enters twice more)


def test_episode_reference_wraps_the_ring():
    ep = rr.Episodes(300)
    s = rr.scenario(300, 24, "on", "three")
    written = 0
    for t in range(24):
        slots, pairs = ep.step(s["rew"][t], s["dones"][t])
        assert len(slots) == len(pairs) == int((s["dones"][t] != 0).sum())
        written += len(pairs)
    assert ep.count == written > 400 and not ep.cr[s["dones"][23] != 0].any()
