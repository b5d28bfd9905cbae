"""On the CPU: the conditions the ragged-count cases of tests/test_hip_env.py rest on, checked with the oracle alone on exactly the
inputs the GPU tests use (tests/env_ragged_ref.py).  A case whose seeds no longer produce the events it is there for -- a time-out
reset, a reset of env N - 1, a step without a reset after one with, ground contact -- fails here, without a GPU."""
import numpy as np
import pytest

from tests import env_ragged_ref as rr


def _oracle(oracle_built, name, n):
    mk, hs, z, meta = rr.pair_inputs(name, n)
    return oracle_built.OracleEnv(mk(), hs), z, meta


def test_counts_sit_off_every_tile():
    assert rr.COUNTS == (1, 7, 17, 47, 65) and all(n % 8 for n in rr.COUNTS)
    assert [n >> 4 for n in rr.COUNTS] == [0, 0, 1, 2, 4] and [n & 15 for n in rr.COUNTS] == [1, 7, 1, 15, 1]      # uint4 part, scalar tail
    assert {c[1] for c in rr.FULL_STEP_CASES} == set(rr.COUNTS) and {c[0] for c in rr.FULL_STEP_CASES} == set(rr.FULL_STEP_ROBOTS)
    assert {c[2] for c in rr.SUBSTEP_CASES} == {1, 17, 47} and {c[0] for c in rr.SUBSTEP_CASES} == {"anymal_c_flat", "cassie", "anymal_c_randomised"}
    # each robot's non-default block shapes (launch_substeps: quadrupeds default to 4 waves and one wave per SIMD, Cassie to 2 waves)
    assert {(c[0], c[1]) for c in rr.SHAPE_CASES} == {("anymal_c_flat", "two_waves"), ("anymal_c_flat", "two_per_cu"), ("cassie", "four_waves")}
    assert {c[2] for c in rr.SHAPE_CASES} == {7, 47} and len(rr.SHAPE_CASES) == 6
    assert {c[1] for c in rr.RESET_IDS_CASES} == {17, 47, 65} and rr.TRAJ_COUNTS == (1, 17, 65)
    assert not any(rr.ragged(n) for n in (64, 96, 128, 133, 256))       # the sizes the file ran before keep their recipes


@pytest.mark.parametrize("name,n", rr.FULL_STEP_CASES)
def test_full_step_cases_hold_their_events(name, n, oracle_built):
    ora, z, meta = _oracle(oracle_built, name, n)
    try:
        state = {}

        def after_reset_all():
            state["lstm"] = float(np.abs(ora.get("lstm_h")).max() + np.abs(ora.get("lstm_c")).max())

        def check(t):
            for key in ("obs", "rew", "root_states", "dof_state", "torques"):
                assert np.isfinite(ora.get(key)).all(), (t, key)
        log = rr.drive_full_step([ora], name, n, z, meta, after_reset_all, check)
        rr.assert_full_step_events(log, n)                  # Cassie included: its ragged cases start CASSIE_DROP lower
        assert state["lstm"] == 0.0                          # reset_all cleared what the recipe had put into the actuator-net state
        assert int(ora.get("fault_total")[0]) == 0
        # the last step keeps the time-out mask of the last step that reset
        last = max(t for t in range(len(log["reset"])) if log["reset"][t].any())
        assert last < len(log["reset"]) - 1
        np.testing.assert_array_equal(ora.get("extras_time_outs").astype(bool), log["time_out"][last])
        assert not np.array_equal(log["time_out"][last], log["time_out"][-1])
    finally:
        ora.close()


@pytest.mark.parametrize("name,z0,n", rr.SUBSTEP_CASES)
def test_substep_cases_touch_the_ground(name, z0, n, oracle_built):
    ora, z, meta = _oracle(oracle_built, name, n)
    try:
        log = rr.drive_substeps([ora], name, z0, n, z, meta)
        rr.assert_substep_events(log, n)
        assert np.isfinite(ora.get("root_states")).all() and np.isfinite(ora.get("dof_state")).all()
        if n > 1:                                            # and not every env: the band rule tells contact from free flight
            assert not np.array(log["in_contact"]).all(0).all()
        if name == "anymal_c_randomised":
            assert ora.setup.to_structs()[0].material_rand == 1 and np.abs(ora.get("material")[n - 1]).sum() > 0
    finally:
        ora.close()


@pytest.mark.parametrize("name,n", rr.RESET_IDS_CASES)
def test_reset_id_lists_reach_the_ragged_tile(name, n, oracle_built):
    ora, z, meta = _oracle(oracle_built, name, n)
    try:
        rng = rr.drive_reset_ids_prologue([ora], name, n, z, meta)
        ids = rr.reset_id_list(rng, n)
        full = n // rr.TILE
        assert ids[0] == 0 and ids[-1] == n - 1 and len(set(ids.tolist())) == len(ids) < n
        assert ((ids >= (full - 1) * rr.TILE) & (ids < full * rr.TILE)).any() and (ids >= full * rr.TILE).any()
        scored = bool(ora.setup.reward_scales)               # (the rough task of this fork has an empty reward table)
        assert (np.abs(ora.get("episode_sums")).sum() > 0) == scored and (ora.get("episode_length") > 0).all()
        ora.call("reset_ids", ids.ctypes.data, len(ids))
        assert int(ora.get("n_reset")[0]) == len(ids) and (ora.get("episode_length")[ids] == 0).all()
        rest = np.setdiff1d(np.arange(n), ids)
        assert (ora.get("episode_length")[rest] > 0).all() and (np.abs(ora.get("extras_episode")).sum() > 0) == scored
        every = np.arange(n, dtype=np.int32)
        ora.call("reset_ids", every.ctypes.data, n)
        assert int(ora.get("n_reset")[0]) == n and (ora.get("episode_length") == 0).all() and not ora.get("episode_sums").any()
    finally:
        ora.close()


@pytest.mark.parametrize("n", rr.TRAJ_COUNTS)
def test_trajectory_cases_hold_their_events(n, oracle_built):
    ora = oracle_built.OracleEnv(rr.traj_inputs(n)())
    try:
        def check(t):
            for key in ("obs", "rew", "tg_state", "trajectory"):
                assert np.isfinite(ora.get(key)).all(), (t, key)
        log = rr.drive_trajectory([ora], n, check=check)
        rr.assert_trajectory_events(log, n)
    finally:
        ora.close()


def test_recipes_at_the_old_sizes_are_unchanged():
    """The sizes the file compared at before this module keep their inputs value for value: clocks, id list."""
    ep = rr.episode_clocks(np.random.default_rng(5), 128, [199, 499, 999, 1000, 1001, 399, 0, 1], 1001)
    want = np.random.default_rng(5).integers(0, 1000, 128)
    want[:8] = [199, 499, 999, 1000, 1001, 399, 0, 1]
    np.testing.assert_array_equal(ep, want)
    ids = rr.reset_id_list(np.random.default_rng(12), 96)
    np.testing.assert_array_equal(ids, np.array(sorted(np.random.default_rng(12).choice(96, 17, replace=False)), np.int32))
    assert rr.FULL_STEP_STEPS == 4
