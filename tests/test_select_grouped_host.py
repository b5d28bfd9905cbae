"""The host side of the grouped selection and of the per-age calibration, without a GPU: the envelope and
workspace queries of lg_select_kth_grouped, the symbols, AgeCalibration's JSON round trip and gathers, trajectory_metrics and the
parsing of coverages into the fractions the kernel computes ranks from."""
import ctypes
import json
import os

import pytest
import torch

from legged_gym_dev_amd import capi
from legged_gym_dev_amd.tube import calibrate as cal
from legged_gym_dev_amd.tube import evaluate as ev

INF = float("inf")


@pytest.fixture(scope="module")
def lib():
    from legged_gym_dev_amd import lib as L
    if not os.path.isfile(L.SO_PATH):
        L.build()
    lib = ctypes.CDLL(L.SO_PATH)
    capi.declare_select_api(lib)
    lib.lg_last_error.restype = ctypes.c_char_p
    return lib


def test_the_library_exports_and_capi_declares_the_entry(lib):
    for name in ("lg_select_grouped_workspace", "lg_select_group_tile", "lg_select_kth_grouped"):
        assert hasattr(lib, name), name
    assert lib.lg_select_grouped_workspace.restype is ctypes.c_int64 and len(lib.lg_select_grouped_workspace.argtypes) == 3
    assert lib.lg_select_group_tile.restype is ctypes.c_int32 and len(lib.lg_select_group_tile.argtypes) == 1
    assert len(lib.lg_select_kth_grouped.argtypes) == 14
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "legged_hip.h")).read()
    assert "#define LG_SELECT_MAX_GROUPS 1024" in text and cal.MAX_GROUPS == 1024


def test_workspace_and_tile_without_a_gpu(lib):
    for B, G, R in ((4096, 16, 1), (1, 1024, 8), (64, 1024, 1), (1, 1, 1)):
        nbytes = lib.lg_select_grouped_workspace(B, G, R)
        gt = lib.lg_select_group_tile(R)
        tiles = -(-G // gt)
        # 1 KiB of bins, a prefix and a rank left per (row, group, rank); a counter per (row, tile)
        assert nbytes == -(-(B * G * R * (1024 + 8) + B * tiles * 4) // 8) * 8 > 0, (B, G, R)
    for R in range(1, 9):
        gt = lib.lg_select_group_tile(R)
        assert gt >= 1 and gt * R * 1024 <= 32 * 1024 < (gt + 1) * R * 1024, R     # the tile fills the workgroup's 32 KiB of bins
    assert lib.lg_select_group_tile(0) == -1 and lib.lg_select_group_tile(9) == -1


def test_workspace_refusals_name_the_field(lib):
    err = lambda: lib.lg_last_error().decode()
    for B, G, R, field in ((0, 1, 1, "B must be 1..4096"), (4097, 1, 1, "B must be 1..4096"), (1, 0, 1, "G must be 1..1024"),
                           (1, 1025, 1, "G must be 1..1024"), (1, 1, 0, "R must be 1..8"), (1, 1, 9, "R must be 1..8"),
                           (65537, 1, 1, "B must be 1..4096"), (1, 1, 65537, "R must be 1..8")):
        assert lib.lg_select_grouped_workspace(B, G, R) == -1 and field in err(), (B, G, R)
    # 65 537 is prime, so no (B, G, R) inside the three ranges has that product: it is refused on the first field out of range (above);
    # the smallest product above 65 536 that the ranges can make is 65 538 = 3641 x 18
    assert lib.lg_select_grouped_workspace(4096, 16, 1) > 0 and lib.lg_select_grouped_workspace(4096, 2, 8) > 0     # B G R = 65 536
    for B, G, R in ((3641, 18, 1), (4096, 17, 1), (4096, 2, 9), (2048, 1024, 1), (1024, 9, 8)):
        want = "R must be 1..8" if R > 8 else "B G R must be at most 65536"
        assert lib.lg_select_grouped_workspace(B, G, R) == -1 and want in err(), (B, G, R)


def test_coverages_become_the_fractions_written():
    assert cal.coverage_fractions(["0.07", 0.9, "0.999", 0.5]) == [(7, 100), (9, 10), (999, 1000), (1, 2)]
    (num, den), = cal.coverage_fractions(["0.07"])
    assert ((99 + 1) * num + den - 1) // den == 7 == cal.conformal_rank(99, "0.07")          # the kernel's integer form; float64 gives 8
    import math
    assert math.ceil((99 + 1) * 0.07) == 8
    for n in (0, 1, 9, 10, 99, 3199, 2 ** 31 - 1):
        for c in ("0.5", "0.9", "0.95", "0.999", "0.07"):
            (num, den), = cal.coverage_fractions([c])
            assert ((n + 1) * num + den - 1) // den == cal.conformal_rank(n, c)
    with pytest.raises(ValueError, match="0.12345678901"):
        cal.coverage_fractions(["0.9", "0.12345678901"])                                     # denominator 10^11 > 2^31 - 1
    assert cal.coverage_fractions(["0.123456789"]) == [(123456789, 10 ** 9)]
    for bad in ("0", "1", "1.5", "-0.1"):
        with pytest.raises(ValueError, match="inside \\(0, 1\\)"):
            cal.coverage_fractions([bad])


def _age_calibration(margin=True):
    offsets = torch.tensor([[[0.5, 1.0], [0.25, INF], [2.0, 3.0]], [[1.5, 2.0], [INF, INF], [4.0, 5.0]]])     # (2 coverages, 3 ages, 2 columns)
    return cal.AgeCalibration([0.5, 0.9], offsets, [20, 1, 7], [[11, 19], [1, 2], [4, 8]],
                              torch.tensor([[0.125, 0.0], [INF, -0.5]]) if margin else None, 16 if margin else None, [9, 16] if margin else None,
                              {"sim_seed": 101, "source": "sim"})


def test_age_calibration_round_trips_through_strict_json(tmp_path):
    c = _age_calibration()
    path = str(tmp_path / cal.AGE_CALIBRATION_NAME)
    assert cal.AGE_CALIBRATION_NAME == "calibration_age.json" and cal.default_age_path("run") == os.path.join("run", "calibration_age.json")
    c.save(path)
    text = open(path).read()
    assert "Infinity" not in text and "NaN" not in text and '"inf"' in text
    json.loads(text, parse_constant=lambda s: pytest.fail(s))
    d = cal.AgeCalibration.load(path)
    assert d.coverages == [0.5, 0.9] and d.max_age == 3 and d.counts == [20, 1, 7] and d.ranks == [[11, 19], [1, 2], [4, 8]]
    assert torch.equal(d.offsets, c.offsets) and torch.equal(d.margin, c.margin) and d.margin_n == 16 and d.margin_ranks == [9, 16]
    assert d.provenance == {"sim_seed": 101, "source": "sim"}
    plain = _age_calibration(margin=False)
    plain.save(path)
    e = cal.AgeCalibration.load(path)
    assert e.margin is None and e.margin_n is None and torch.equal(e.offsets, c.offsets)
    with pytest.raises(ValueError, match="no trajectory margin"):
        e.offset_at(torch.tensor([0]), 0.5, trajectory=True)
    assert len(c.lines()) == 2 * 3 * 2 + 2 * 2 and len(plain.lines()) == 12


def test_a_nan_offset_is_refused_and_named():
    offsets = torch.zeros(2, 3, 2)
    offsets[1, 2, 0] = float("nan")
    with pytest.raises(ValueError, match="coverage 0.9, age 2, column 0"):
        cal.AgeCalibration([0.5, 0.9], offsets, [1, 1, 1], [[1, 1]] * 3)
    with pytest.raises(ValueError, match="NaN margin at coverage 0.5, column 1"):
        cal.AgeCalibration([0.5, 0.9], torch.zeros(2, 3, 2), [1, 1, 1], [[1, 1]] * 3, torch.tensor([[0.0, float("nan")], [0.0, 0.0]]), 4, [3, 4])


def test_offset_at_clamps_the_age():
    c = _age_calibration()
    age = torch.tensor([[0, 1, 2, 3, 100], [2, 2, 0, -1, 1]])
    q = c.offset_at(age, 0.5)
    assert tuple(q.shape) == (2, 5, 2)
    assert q[0].tolist() == [[0.5, 1.0], [0.25, INF], [2.0, 3.0], [2.0, 3.0], [2.0, 3.0]]
    assert q[1, 3].tolist() == [0.5, 1.0]
    assert c.offset_at(age, 0.5, trajectory=True)[0, 2].tolist() == [2.125, 3.0]
    assert c.offset_at(torch.tensor(7), 0.9).tolist() == [4.0, 5.0]
    with pytest.raises(KeyError):
        c.offset_at(age, 0.95)
    fw = torch.zeros(2, 5, 2)
    w = torch.full((2, 5, 2), 1.0)
    assert torch.equal(c.apply(fw, age, 0.5), q)
    assert torch.equal(c.covers(fw, w, age, 0.5), w <= q)
    assert torch.equal(c.covers(fw, w, age, 0.5, trajectory=True), (w - q) <= torch.tensor([0.125, 0.0]))
    assert bool(c.covers(fw, w, age, 0.9, trajectory=True)[..., 0].all())                     # an infinite margin covers everything


def test_trajectory_metrics_on_hand_made_cases():
    covered = torch.tensor([[[1, 1], [1, 0], [1, 1]],        # env 0: column 1 misses step 1
                            [[1, 1], [0, 0], [1, 1]],        # env 1: step 1 misses both, but is done
                            [[0, 1], [1, 1], [1, 1]],        # env 2: column 0 misses step 0
                            [[1, 1], [1, 1], [1, 1]]]).bool()
    done = torch.zeros(4, 3, dtype=torch.bool)
    assert ev.trajectory_metrics(covered, done) == {"envs": 4, "trajectory_success_rate": [0.5, 0.5]}
    done[1, 1] = True
    assert ev.trajectory_metrics(covered, done) == {"envs": 4, "trajectory_success_rate": [0.75, 0.75]}
    done[0, 1] = True
    assert ev.trajectory_metrics(covered, done.to(torch.uint8)) == {"envs": 4, "trajectory_success_rate": [0.75, 1.0]}
    done[:] = True                                          # nothing kept: nothing missed
    assert ev.trajectory_metrics(covered, done)["trajectory_success_rate"] == [1.0, 1.0]
    with pytest.raises(ValueError, match="shapes"):
        ev.trajectory_metrics(covered, done[:, :2])


def test_age_groups():
    done = torch.zeros(2, 8, dtype=torch.bool)
    done[0, 4] = True
    reseed = ev.reseed_mask(done, 3)
    group, G = cal.age_groups(done, reseed)
    assert G == 3 and group.dtype == torch.int32
    assert group.tolist() == [[0, 1, 2, 0, -1, 0, 1, 2], [0, 1, 2, 0, 1, 2, 0, 1]]
    group, G = cal.age_groups(done, ev.reseed_mask(done, None), 4)
    assert G == 4 and group.tolist() == [[0, 1, 2, 3, -1, 0, 1, 2], [0, 1, 2, 3, 3, 3, 3, 3]]
    group, G = cal.age_groups(done, ev.reseed_mask(done, None))
    assert G == 8 and group[1].tolist() == list(range(8))
    with pytest.raises(ValueError, match="max_age"):
        cal.age_groups(done, reseed, 1025)
