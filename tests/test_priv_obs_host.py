"""Host side of the privileged observations (envs/base/privileged_obs.py, lg_priv_obs_check): widths, refusals that name their
field, how env.num_privileged_obs is resolved, the cfg -> lg_priv_cfg mapping, the configuration contract, and a reference-style
cfg class without the section.  No GPU: lg_priv_obs_check is host code."""
import ctypes
import os
import types

import pytest

from legged_gym_dev_amd import capi
from legged_gym_dev_amd.envs.base import cfg_contract as cc
from legged_gym_dev_amd.envs.base import privileged_obs as po
from legged_gym_dev_amd.envs.base.env_setup import EnvSetup, sim_dt_float
from legged_gym_dev_amd.model.robot_model import compile_model, resolve_model
from legged_gym_dev_amd.utils.helpers import class_to_dict, get_args, update_cfg_from_args
from tests import harness

FLAT = dict(num_obs=48, num_actions=12, num_feet=4, num_pen=8, num_height_points=0, measure_heights=0)


@pytest.fixture(scope="module")
def lib():
    import torch  # noqa: F401  (shares the HIP runtime instance)
    from legged_gym_dev_amd import lib as L
    if not os.path.isfile(L.SO_PATH):
        L.build()
    return capi.declare_priv_obs_api(ctypes.CDLL(L.SO_PATH))


def _struct(kinds, scales=None):
    c = capi.lg_priv_cfg()
    c.num_terms = len(kinds)
    for k, kind in enumerate(kinds[:capi.PRIV_MAX_TERMS]):
        c.terms[k].kind, c.terms[k].scale = kind, (scales[k] if scales else 1.0)
    return c


def _check(lib, c, d):
    """(rc, width, the library's sentence without its prefix)"""
    w = ctypes.c_int32(-7)
    rc = lib.lg_priv_obs_check(ctypes.byref(c), d["num_obs"], d["num_actions"], d["num_feet"], d["num_pen"], d["num_height_points"],
                               d["measure_heights"], ctypes.byref(w))
    msg = lib.lg_last_error().decode() if rc else ""
    assert rc in (0, -1) and (rc == 0 or msg.startswith("lg_priv_obs: "))
    return rc, w.value, msg[len("lg_priv_obs: "):]


def _setup(name):
    z, meta = harness.load_fixture(name)
    return harness.make_setup(name, z, meta)


@pytest.mark.parametrize("task,want", [
    # obs, friction, base_mass, material, 3 F, F, F, penalised bodies, A, [H], progress
    ("anymal_c_flat", dict(obs=48, friction=1, base_mass=1, material=4, feet_contact_forces=12, feet_contact=4, feet_air_time=4,
                           body_contact=8, torques=12, episode_progress=1)),
    ("anymal_c_rough", dict(obs=235, friction=1, base_mass=1, material=4, feet_contact_forces=12, feet_contact=4, feet_air_time=4,
                            body_contact=8, torques=12, heights=187, episode_progress=1)),
    ("cassie", dict(obs=169, friction=1, base_mass=1, material=4, feet_contact_forces=6, feet_contact=2, feet_air_time=2,
                    body_contact=0, torques=12, heights=121, episode_progress=1)),      # no penalised body: the term is refused
    ("anymal_c_flat_trajectory", dict(obs=65, friction=1, base_mass=1, material=4, feet_contact_forces=12, feet_contact=4,
                                      feet_air_time=4, body_contact=8, torques=12, episode_progress=1))])
def test_widths_of_every_term_on_the_four_kinds_of_env(lib, task, want):
    setup, cfg = _setup(task)
    d = po.dims_of(setup)
    assert want["body_contact"] == len(setup.penalised_contact_indices) and want["feet_contact"] == len(setup.feet_indices)
    if want["body_contact"] == 0:
        cfg.privileged_obs.terms = ["obs", "body_contact"]
        with pytest.raises(ValueError, match="terms\\[1\\].kind: the term 'body_contact' has no entries"):
            po.PrivilegedObsSpec.from_cfg(cfg, setup)
        want = {k: v for k, v in want.items() if k != "body_contact"}
    cfg.privileged_obs.terms = list(want)
    spec = po.PrivilegedObsSpec.from_cfg(cfg, setup)
    assert spec.widths() == want and spec.width == sum(want.values())
    offs = spec.offsets()
    assert list(offs.values()) == [sum(list(want.values())[:k]) for k in range(len(want))]
    rc, W, msg = _check(lib, spec.to_struct(), d)
    assert (rc, W) == (0, spec.width), msg
    for name, w in want.items():                               # and each term alone
        rc, W, msg = _check(lib, _struct([capi.PRIV_TERMS.index(name)]), d)
        assert (rc, W) == (0, w), (name, msg)


@pytest.mark.parametrize("c,d,field", [
    (_struct([0, 99]), FLAT, "terms[1].kind = 99"),                                      # unknown kind
    (_struct([-1]), FLAT, "terms[0].kind = -1"),
    (_struct([1, 0, 1]), FLAT, "terms[2].kind: the term 'friction' appears twice (also terms[0])"),
    (_struct([0, capi.PRIV_TERMS.index("heights")]), FLAT, "terms[1].kind: 'heights' needs an env with measure_heights"),
    (_struct([0] * 17), FLAT, "num_terms = 17 must lie in 1..16"),                       # more than LG_PRIV_MAX_TERMS
    (_struct([]), FLAT, "num_terms = 0 must lie in 1..16"),
    (_struct([0, capi.PRIV_TERMS.index("heights")]), dict(FLAT, num_obs=1000, num_height_points=187, measure_heights=1),
     "width = 1187 exceeds LG_PRIV_MAX_WIDTH = 1024"),
    (_struct([1], [float("nan")]), FLAT, "terms[0].scale is not finite"),
    (_struct([capi.PRIV_TERMS.index("body_contact")]), dict(FLAT, num_pen=0), "terms[0].kind: the term 'body_contact' has no entries"),
])
def test_every_refusal_names_its_field(lib, c, d, field):
    rc, W, msg = _check(lib, c, d)
    assert rc == -1 and W == -7 and field in msg, msg             # the width is left alone on a refusal
    assert po.refusal(c, **d) == msg                              # the sentence PrivilegedObsSpec.from_cfg raises with


def test_accepted_rows_and_null_arguments(lib):
    for kinds in ([0], [10, 3, 1], list(range(9)) + [10]):
        c = _struct(kinds, [0.5 + k for k in range(len(kinds))])
        assert po.refusal(c, **FLAT) is None and _check(lib, c, FLAT)[0] == 0
    assert lib.lg_priv_obs_check(None, 48, 12, 4, 8, 0, 0, None) == -1 and lib.lg_last_error().decode() == "lg_priv_obs: cfg is null"
    assert lib.lg_priv_obs_check(ctypes.byref(_struct([0])), 48, 12, 4, 8, 0, 0, None) == 0      # width may be NULL


def test_from_cfg_refuses_in_the_cfgs_words():
    setup, cfg = _setup("anymal_c_flat")
    for terms, word in ((["obs", "fricton"], "fricton"), (["obs", "obs"], "appears twice"), (["heights"], "measure_heights"),
                        (["obs"] * 17, "num_terms = 17")):
        cfg.privileged_obs.terms = terms
        with pytest.raises(ValueError, match="cfg.privileged_obs.*" + word):
            po.PrivilegedObsSpec.from_cfg(cfg, setup)


def test_num_privileged_obs_is_resolved_from_the_terms():
    from legged_gym_dev_amd.envs.base.base_task import BaseTask
    setup, cfg = _setup("anymal_c_flat")
    # no terms: today's behaviour, including the refusal of a bare width
    assert po.PrivilegedObsSpec.from_cfg(cfg, setup).terms == ()
    assert BaseTask(cfg, None, None, "cuda:0", True).num_privileged_obs is None
    cfg.env.num_privileged_obs = 54
    with pytest.raises(NotImplementedError, match="privileged observations"):
        BaseTask(cfg, None, None, "cuda:0", True)
    # terms: None becomes W, W is accepted, anything else lists every term's width
    cfg.privileged_obs.terms = ["obs", "friction", "base_mass", "feet_contact"]
    spec = po.PrivilegedObsSpec.from_cfg(cfg, setup)
    assert BaseTask(cfg, None, None, "cuda:0", True).privileged_obs_buf is None       # the width no longer refuses; LeggedRobot binds the view
    assert spec.resolve_num_privileged_obs(None) == 54 and spec.resolve_num_privileged_obs(54) == 54
    with pytest.raises(ValueError) as e:
        spec.resolve_num_privileged_obs(55)
    for part in ("num_privileged_obs = 55", "54 columns", "obs 48", "friction 1", "base_mass 1", "feet_contact 4"):
        assert part in str(e.value), str(e.value)


def test_cfg_maps_onto_the_struct_term_by_term():
    setup, cfg = _setup("anymal_c_rough")
    cfg.privileged_obs.terms = ["heights", "friction", "obs", "episode_progress"]
    cfg.privileged_obs.scales.friction, cfg.privileged_obs.scales.heights = 2.5, -0.25
    spec = po.PrivilegedObsSpec.from_cfg(cfg, setup)
    c = spec.to_struct()
    assert ctypes.sizeof(capi.lg_priv_cfg) == 8 + 8 * capi.PRIV_MAX_TERMS and ctypes.sizeof(capi.lg_priv_term) == 8
    assert c.num_terms == 4 and [c.terms[k].kind for k in range(4)] == [9, 1, 0, 10]
    assert [c.terms[k].scale for k in range(4)] == [-0.25, 2.5, 1.0, 1.0]
    assert spec.dims == dict(num_obs=235, num_actions=12, num_feet=4, num_pen=8, num_height_points=187, measure_heights=1)
    assert spec.offsets() == {"heights": 0, "friction": 187, "obs": 188, "episode_progress": 423} and spec.width == 424


def test_struct_sizes_match_the_header(lib):
    import subprocess
    import tempfile
    src = '#include <stdio.h>\n#include "legged_hip.h"\nint main(){printf("%zu %zu %d %d %d\\n",sizeof(lg_priv_term),' \
          'sizeof(lg_priv_cfg),LG_PRIV_MAX_TERMS,LG_PRIV_MAX_WIDTH,LG_PRIV_NUM_KINDS);return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(harness.ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        out = [int(v) for v in subprocess.check_output([os.path.join(d, "t")]).decode().split()]
    assert out == [ctypes.sizeof(capi.lg_priv_term), ctypes.sizeof(capi.lg_priv_cfg), capi.PRIV_MAX_TERMS, capi.PRIV_MAX_WIDTH,
                   len(capi.PRIV_TERMS)]


def test_every_new_cfg_leaf_is_in_the_contract_as_read_by_the_env():
    from legged_gym_dev_amd.envs.base.legged_robot_config import LeggedRobotCfg
    paths = [p for p, _ in cc.leaves(class_to_dict(LeggedRobotCfg())) if p.startswith("privileged_obs.")]
    assert sorted(paths) == sorted(["privileged_obs.terms"] + ["privileged_obs.scales." + t for t in capi.PRIV_TERMS])
    for p in paths:
        row = cc.lookup(p)
        assert row is not None and row[1] == cc.CONSUMED and row[2].startswith("env:"), p
    cfg = LeggedRobotCfg()
    assert cfg.privileged_obs.terms == [] and all(getattr(cfg.privileged_obs.scales, t) == 1.0 for t in capi.PRIV_TERMS)


def test_a_reference_style_cfg_without_the_section_builds_a_spec_of_no_terms():
    full = harness.make_cfg("anymal_c_flat")
    cfg = types.SimpleNamespace(**{k: getattr(full, k) for k in dir(full)
                                   if not k.startswith("_") and k != "privileged_obs" and not callable(getattr(full, k))})
    assert not hasattr(cfg, "privileged_obs")
    cm = compile_model(resolve_model("", "anymal_c"))
    setup = EnvSetup(cfg, cm, sim_dt_float(cfg.sim.dt))           # the contract walk accepts the tree without the section
    spec = po.PrivilegedObsSpec.from_cfg(cfg, setup)
    assert spec.terms == () and spec.width == 0 and spec.widths() == {}
    # --privileged_obs on such a cfg makes the section, with unit scales
    args = get_args(["--task", "anymal_c_flat", "--privileged_obs", "obs, friction,base_mass"])
    update_cfg_from_args(cfg, None, args)
    spec = po.PrivilegedObsSpec.from_cfg(cfg, setup)
    assert spec.terms == ("obs", "friction", "base_mass") and spec.scales == (1.0, 1.0, 1.0) and spec.width == 50
    cc.enforce(cfg)


def test_train_argument_reaches_the_cfg():
    cfg = harness.make_cfg("anymal_c_flat")
    update_cfg_from_args(cfg, None, get_args(["--task", "anymal_c_flat"]))
    assert cfg.privileged_obs.terms == []
    update_cfg_from_args(cfg, None, get_args(["--task", "anymal_c_flat", "--privileged_obs", "obs,friction,feet_air_time"]))
    assert cfg.privileged_obs.terms == ["obs", "friction", "feet_air_time"]
