"""The C-ABI library loads without a GPU and exports every symbol include/legged_hip.h declares;
without a GPU the product path fails loudly instead of falling back."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "legged_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(lg_[a-z_0-9]+)\s*\(", text)))


@pytest.fixture(scope="module")
def lib():
    import torch  # noqa: F401  (shares the HIP runtime instance)
    from legged_gym_dev_amd import lib as L
    if not os.path.isfile(L.SO_PATH):
        L.build()
    return ctypes.CDLL(L.SO_PATH)


def test_header_declares_the_expected_surface():
    syms = _declared_symbols()
    for must in ("lg_create", "lg_step", "lg_post_physics_step", "lg_simulate", "lg_compute_torques", "lg_ppo_create",
                 "lg_ppo_act", "lg_ppo_minibatch_backward", "lg_ppo_minibatch_step", "lg_last_error"):
        assert must in syms
    assert len(syms) >= 30


def test_library_exports_every_declared_symbol(lib):
    missing = [s for s in _declared_symbols() if not hasattr(lib, s)]
    assert not missing, missing


def test_ctypes_structs_match_header_sizes(lib):
    from legged_gym_dev_amd import capi
    # layout guard: sizes computed from the header with the C compiler must equal the ctypes mirrors
    import subprocess
    import tempfile
    src = '#include <stdio.h>\n#include "legged_hip.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu\\n",sizeof(lg_model),' \
          'sizeof(lg_cfg),sizeof(lg_buffers),sizeof(lg_ppo_cfg),sizeof(lg_ppo_buffers),sizeof(lg_stage));return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        out = subprocess.check_output([os.path.join(d, "t")]).decode().split()
    got = [ctypes.sizeof(c) for c in (capi.lg_model, capi.lg_cfg, capi.lg_buffers, capi.lg_ppo_cfg, capi.lg_ppo_buffers, capi.lg_stage)]
    assert [int(v) for v in out] == got


def test_no_gpu_means_loud_failure_not_fallback(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from tests import harness
    z, meta = harness.load_fixture("anymal_c_flat")
    setup, _ = harness.make_setup("anymal_c_flat", z, meta)
    from legged_gym_dev_amd.lib import HipEnvCore, LeggedHipError
    with pytest.raises(LeggedHipError):
        HipEnvCore(setup, None, "cuda:0")
    with pytest.raises(LeggedHipError):
        HipEnvCore(setup, None, "cpu")


# ---------------------------------------------------------------- every prototype of the header against its ctypes declaration
# Names Python declares (or probes) that the header does not: two test hooks of the learner, and lg_plan_score_scenes as the marker
# of a library built before lg_plan_call.  Listed so that the set cannot grow unnoticed.  (lg_select_chunk and lg_select_group_tile
# return int32_t and are in the header: the loop over its prototypes covers them, restype included.)
NOT_IN_HEADER = {"lg_ppo_debug_bucket_extents", "lg_ppo_debug_mb_sets", "lg_plan_score_scenes"}


def _header_prototypes():
    text = open(os.path.join(ROOT, "include", "legged_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return {name: (" ".join(ret.split()), params)
            for ret, name, params in re.findall(r"(?m)^[ \t]*((?:const[ \t]+)?\w+[ \t]*\*?)[ \t]*\b(lg_\w+)[ \t]*\(([^)]*)\)\s*;", text)}


_C_CLASS = {"int": "i32", "int32_t": "i32", "uint32_t": "i32", "int64_t": "i64", "uint64_t": "i64", "size_t": "i64", "float": "float",
            "double": "double"}


def _class_of_c(param):
    if "*" in param:
        return "pointer"
    words = [w for w in param.split() if w != "const"]
    return _C_CLASS[words[0]]


def _class_of_ctypes(t):
    if t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, (ctypes._Pointer, ctypes.Array)):
        return "pointer"
    return {ctypes.c_int32: "i32", ctypes.c_uint32: "i32", ctypes.c_int64: "i64", ctypes.c_uint64: "i64", ctypes.c_float: "float",
            ctypes.c_double: "double"}[t]


def test_argtypes_match_every_prototype_of_the_header():
    """ctypes checks nothing at a call: as many argtypes as the prototype has parameters, per position the same class -- pointer,
    32-bit integer, 64-bit integer, float, double -- the restype of the entries that do not return int, and no prototype without
    a declaration."""
    from legged_gym_dev_amd import capi
    from legged_gym_dev_amd.lib import load
    lib = load()
    for declare in (capi.declare_cmdtrack_api, capi.declare_priv_obs_api, capi.declare_obs_hist_api, capi.declare_obs_norm_api):
        declare(lib)
    protos = _header_prototypes()
    assert len(protos) >= 154 and set(protos) == set(_declared_symbols())
    bad = []
    for name, (ret, params) in sorted(protos.items()):
        fn = getattr(lib, name)
        want = [] if params.strip() in ("", "void") else [_class_of_c(q.strip()) for q in params.split(",")]
        if fn.argtypes is None:
            bad.append(f"{name}: no argtypes")
        elif [_class_of_ctypes(t) for t in fn.argtypes] != want:
            bad.append(f"{name}: {[_class_of_ctypes(t) for t in fn.argtypes]} for {want}")
        want_res = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "const char *": ctypes.c_char_p}[ret]
        if fn.restype is not want_res:
            bad.append(f"{name}: restype {fn.restype} for {ret}")
    assert not bad, bad
    # what Python names beyond the header: exactly the listed ones
    src = "".join(open(os.path.join(ROOT, "legged_gym_dev_amd", f)).read() for f in ("capi.py", "lib.py"))
    named = set(re.findall(r"\blg_[a-z_0-9]+\b", src)) - {n for n in re.findall(r"class (lg_\w+)", src)}
    callable_extra = {n for n in named if n not in protos and (hasattr(lib, n) or n in NOT_IN_HEADER)}
    assert callable_extra == NOT_IN_HEADER, sorted(callable_extra ^ NOT_IN_HEADER)


# ---------------------------------------------------------------- no source file declares a function it does not define
# Cross-file functions are declared once, in a header both sides include (csrc/lg_internal.h, the families' *_device.h,
# ppo_launch.h, ppo_learner.h): the compiler then checks every call against the definition.  A prototype written out again in a
# .hip / .cpp would link against whatever the definition has become.  The scanner reads declarations only.
_SKIP_HEAD = {"typedef", "using", "static_assert", "return", "template", "friend"}
_NOT_NAMES = {"__attribute__", "__launch_bounds__", "__align__", "alignas", "noexcept", "decltype", "sizeof"}


def _strip(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r'extern\s+"C"', "extern_C", text)
    text = re.sub(r'"(?:\\.|[^"\\\n])*"', '""', text)
    text = re.sub(r"'(?:\\.|[^'\\\n])'", "' '", text)
    text = re.sub(r"^[ \t]*#(?:[^\n]*\\\n)*[^\n]*", " ", text, flags=re.M)    # preprocessor lines, continued ones included
    return text


def _callee(stmt):
    """Name in front of the last top-level parenthesis group of stmt (None if stmt has none or it is no function declarator)."""
    depth, groups, start = 0, [], None
    for i, ch in enumerate(stmt):
        if ch == "(":
            if depth == 0:
                start = i
            depth += 1
        elif ch == ")":
            depth -= 1
            if depth == 0:
                groups.append((start, i))
    for start, _ in reversed(groups):
        m = re.search(r"([A-Za-z_][\w:]*)\s*$", stmt[:start])
        if not m:
            return None
        if m.group(1) in _NOT_NAMES:
            continue
        head = stmt[:m.start()].strip()
        if not head or "=" in head or head.split()[0] in _SKIP_HEAD:   # a call / macro use, an initialiser, a typedef
            return None
        return m.group(1)
    return None


def scan_prototypes(text):
    """(declared, defined): names of the functions a C++ source declares without a body (a declaration ending in ');' at file scope or
    inside an extern "C" / namespace block) and of those it defines there."""
    text = _strip(text)
    declared, defined = [], set()
    depth, stmt, opened = 0, "", []          # opened: per open brace, whether it counts as a nesting level
    for ch in text:
        if ch == "{":
            s = stmt.strip()
            transparent = depth == 0 and (s == "extern_C" or re.fullmatch(r"(inline\s+)?namespace(\s+\w+)?", s) is not None)
            if depth == 0 and not transparent and re.search(r"\)\s*(const|noexcept|\s)*$", s):
                name = _callee(s)
                if name:
                    defined.add(name)
            opened.append(not transparent)
            depth += not transparent
            stmt = ""
        elif ch == "}":
            if opened and opened.pop():
                depth -= 1
            stmt = ""
        elif ch == ";":
            s = re.sub(r"^extern_C\s+", "", stmt.strip())
            if depth == 0 and re.search(r"\)\s*(const|noexcept|\s)*$", s):
                name = _callee(s)
                if name:
                    declared.append(name)
            stmt = ""
        elif depth == 0:
            stmt += ch
    return declared, defined


def foreign_prototypes(text):
    """Functions the source declares but does not define."""
    declared, defined = scan_prototypes(text)
    return sorted({n for n in declared if n not in defined})


def test_no_source_declares_a_function_it_does_not_define():
    import glob
    csrc = os.path.join(ROOT, "legged_gym_dev_amd", "csrc")
    files = sorted(glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.cpp")))
    assert len(files) >= 29
    bad = {os.path.basename(f): foreign_prototypes(open(f).read()) for f in files}
    assert not {f: v for f, v in bad.items() if v}, bad
    # the scanner sees definitions where they are: a file with launchers defines them
    assert "ppok_gather" in scan_prototypes(open(os.path.join(csrc, "ppo_kernels.hip")).read())[1]
    # negative control: a prototype over two lines inside an extern "C" block, next to a definition of something else
    ctl = 'extern "C" {\nvoid ppok_gather(const PpoDev *P, int mb,\n                 hipStream_t s);\n}\nint f() { return 0; }\n'
    assert foreign_prototypes(ctl) == ["ppok_gather"]
    assert foreign_prototypes("void g(int a);\nvoid g(int a) { (void)a; }\nstatic int h(void);\n") == ["h"]
