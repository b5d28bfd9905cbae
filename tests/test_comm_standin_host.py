"""No GPU: the RCCL stand-in of the multi-rank tests (tests/comm_standin) and the loader override that reaches it.

LG_RCCL_LIB makes legged_gym_dev_amd/csrc/comm_api.cpp resolve RCCL's entry points from exactly the named file, with no fallback.
The library caches that handle per process, so every check runs in a child process of its own.  What the stand-in computes on the
device is tests/test_hip_comm_standin.py's business."""
import os
import subprocess
import sys

from tests import comm_standin_worker as csw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_ID_CHILD = """
import ctypes as C, sys
sys.path.insert(0, %r)
from legged_gym_dev_amd.lib import load
lib = load()
lib.lg_comm_get_unique_id.argtypes = [C.c_void_p]
lib.lg_last_error.restype = C.c_char_p
for _ in range(2):
    buf = (C.c_char * 128)()
    rc = lib.lg_comm_get_unique_id(buf)
    print("rc", rc)
    print("id", bytes(buf).hex())
    print("error", lib.lg_last_error().decode())
""" % ROOT


def _run(code, **env):
    p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    return p.stdout.splitlines()


def _field(lines, key):
    return [ln.split(" ", 1)[1] if " " in ln else "" for ln in lines if ln.split(" ", 1)[0] == key]


def test_standin_exports_what_comm_api_resolves():
    so = csw.build_standin()
    out = _run(f"import ctypes\nso = ctypes.CDLL({so!r})\nprint('missing', [n for n in {list(csw.EXPORTS)!r} if not hasattr(so, n)])\n")
    assert _field(out, "missing") == ["[]"], out
    # ... and nothing else but its own test controls: every other function of it is internal
    nm = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    funcs = {ln.split()[2] for ln in nm.splitlines() if len(ln.split()) == 3 and ln.split()[1] == "T"}
    assert {f for f in funcs if not f.startswith("standin_")} == set(csw.EXPORTS), funcs


def test_loader_override_reaches_the_standin():
    out = _run(_ID_CHILD, LG_RCCL_LIB=csw.build_standin())
    assert _field(out, "rc") == ["0", "0"], out
    a, b = (bytes.fromhex(x) for x in _field(out, "id"))
    assert a != b and a.startswith(b"standin") and b.startswith(b"standin") and len(a) == 128


def test_loader_override_has_no_fallback():
    missing = os.path.join(ROOT, "tests", "comm_standin", "_build", "no_such_librccl.so")
    out = _run(_ID_CHILD, LG_RCCL_LIB=missing)
    assert all(rc != "0" for rc in _field(out, "rc")) and len(_field(out, "rc")) == 2, out
    assert all(missing in e for e in _field(out, "error")), out
