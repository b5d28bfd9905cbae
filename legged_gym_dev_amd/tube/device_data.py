"""Tube datasets built on the device (lg_tube_rows_build / lg_tube_horizon_build): the rows of tube/data.py
from records that never leave HBM.

    build_rows(records, kind, ...)      (data, target) device tensors from a record dict {z, pz_x, v, done} (host or device)
    from_records(cls, records, ...)     the dataset classes of tube/data.py holding device tensors
    SimTubeDataset(sim, kind, ...)      a HipRomSim and the records of its last epochs; update() collects fresh ones

The rule is data.py's, bit for bit; there is no CPU fallback: without the library or a GPU these raise.
"""
import ctypes as C
from collections import deque

import numpy as np
import torch

from .. import capi
from . import data as td

_KIND_OF = {td.ScalarTubeDataset: "scalar", td.VectorTubeDataset: "vector", td.ErrorDynamicsDataset: "error_dynamics",
            td.LevelScalarTubeDataset: "scalar", td.LevelVectorTubeDataset: "vector"}


def make_spec(kind, N, dN, recursive, n, m, T, n_env, compact=True, mark_last_env=True, epoch_envs=None):
    """lg_tube_rows_spec; kind: scalar | vector | error_dynamics, or a level kind (its base kind's rows)."""
    kind = td.LEVEL_KINDS.get(kind, kind)
    if kind not in capi.TUBE_ROWS_KIND:
        raise ValueError(f"kind {kind!r} has no per-step rows; one of {sorted(capi.TUBE_ROWS_KIND)}")
    return capi.lg_tube_rows_spec(kind=capi.TUBE_ROWS_KIND[kind], N=int(N), dN=int(dN), recursive=int(bool(recursive)), n=int(n), m=int(m),
                                  T=int(T), n_env=int(n_env), compact=int(bool(compact)), mark_last_env=int(bool(mark_last_env)),
                                  epoch_envs=int(n_env if epoch_envs is None else epoch_envs))


def spec_dims(lib, spec):
    """(input_dim, output_dim) of the spec's rows; ValueError, naming the field, outside the envelope."""
    i, o = C.c_int32(), C.c_int32()
    if lib.lg_tube_rows_dims(C.byref(spec), C.byref(i), C.byref(o)) != 0:
        raise ValueError(lib.lg_last_error().decode())
    return i.value, o.value


def _device(records, device):
    if device is not None:
        return torch.device(device)
    z = records["z"]
    return z.device if isinstance(z, torch.Tensor) and z.is_cuda else torch.device("cuda:0")


def device_records(records, device=None):
    """{z, pz_x, v (float32), done (uint8)} as contiguous tensors on the device; device tensors pass through without a copy."""
    from ..lib import LeggedHipError
    dev = _device(records, device)
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise LeggedHipError("the device dataset builder needs a GPU device (no CPU fallback); got " + str(dev))
    out = {k: torch.as_tensor(records[k]).to(dev, torch.float32).contiguous() for k in ("z", "pz_x", "v")}
    done = torch.as_tensor(records["done"]) if "done" in records else torch.zeros(out["v"].shape[:2], dtype=torch.uint8)
    done = done.to(dev).contiguous()
    out["done"] = done.view(torch.uint8) if done.dtype == torch.bool else done.ne(0).to(torch.uint8)
    z, pz, v = out["z"], out["pz_x"], out["v"]
    if z.dim() != 3 or pz.shape != z.shape or v.dim() != 3 or v.shape[0] != z.shape[0] or v.shape[1] + 1 != z.shape[1] \
            or tuple(out["done"].shape) != tuple(v.shape[:2]):
        raise ValueError(f"records must be z, pz_x (n_env, T+1, n), v (n_env, T, m), done (n_env, T); got z {tuple(z.shape)}, "
                         f"pz_x {tuple(pz.shape)}, v {tuple(v.shape)}, done {tuple(out['done'].shape)}")
    return out


def build_rows_into(spec, rec, data, target, n_rows):
    """Queue lg_tube_rows_build on the current stream: rec from device_records; data, target with room for n_env T rows; n_rows a
    device int64 tensor of one element.  Waits for nothing.  Returns the workspace (torch's allocator reuses it in stream order)."""
    from ..lib import LeggedHipError, load
    lib = load()
    nbytes = lib.lg_tube_rows_workspace(C.byref(spec))
    if nbytes < 0:
        raise ValueError(lib.lg_last_error().decode())
    dev = rec["z"].device
    ws = torch.empty(max(1, (nbytes + 7) // 8), dtype=torch.int64, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    with torch.cuda.device(dev):
        rc = lib.lg_tube_rows_build(C.byref(spec), p(rec["z"]), p(rec["pz_x"]), p(rec["v"]), p(rec["done"]), p(data), p(target), p(n_rows),
                                    p(ws), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    if rc != 0:
        raise LeggedHipError(f"lg_tube_rows_build failed ({rc}): {lib.lg_last_error().decode()}")
    return ws


def build_rows(records, kind, N=1, dN=1, recursive=False, compact=True, mark_last_env=True, epoch_envs=None, device=None):
    """The rows DATASETS[kind] builds from `records`, on the device.  compact: (rows, input_dim), (rows, output_dim) without the done
    rows, in (env, time) order -- one 8-byte read-back trims them to the rows written; mark_last_env counts every step of the last
    env of each epoch_envs envs (default: of all) as done, construct_dataset's per-epoch quirk.  Not compact: every row, as
    sequences() shapes them, (n_env, T, input_dim) and (n_env, T, output_dim)."""
    from ..lib import load
    rec = device_records(records, device)
    n_env, T, m = rec["v"].shape
    spec = make_spec(kind, N, dN, recursive, rec["z"].shape[2], m, T, n_env, compact, mark_last_env, epoch_envs)
    I, O = spec_dims(load(), spec)
    dev = rec["z"].device
    data = torch.empty((n_env * T, I), dtype=torch.float32, device=dev)
    target = torch.empty((n_env * T, O), dtype=torch.float32, device=dev)
    n_rows = torch.zeros(1, dtype=torch.int64, device=dev)
    build_rows_into(spec, rec, data, target, n_rows)
    if not compact:
        return data.reshape(n_env, T, I), target.reshape(n_env, T, O)
    rows = int(n_rows.item())
    return data[:rows], target[:rows]


def build_horizon(records, H_rev, device=None):
    """ScalarHorizonTubeDataset.from_folder's w (n_env, T + H_rev), z without its position (n_env, T + H_rev, n - 2) and v
    (n_env, T + H_rev, m), on the device."""
    from ..lib import LeggedHipError, load
    lib = load()
    rec = device_records(records, device)
    n_env, T, m = rec["v"].shape
    n, dev, Tp = rec["z"].shape[2], rec["z"].device, T + int(H_rev)
    f = dict(dtype=torch.float32, device=dev)
    w, z, v = torch.empty((n_env, Tp), **f), torch.empty((n_env, Tp, n - 2), **f), torch.empty((n_env, Tp, m), **f)
    p = lambda t: C.c_void_p(t.data_ptr())
    with torch.cuda.device(dev):
        rc = lib.lg_tube_horizon_build(p(rec["z"]), p(rec["pz_x"]), p(rec["v"]), n_env, T, n, m, int(H_rev), p(w), p(z) if n > 2 else None,
                                       p(v), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    if rc != 0:
        raise (ValueError if rc == -1 else LeggedHipError)(f"lg_tube_horizon_build failed ({rc}): {lib.lg_last_error().decode()}")
    return w, z, v


def from_records(cls, records, N=1, dN=1, recursive=False, H_fwd=50, H_rev=10, mark_last_env=True, epoch_envs=None, device=None):
    """cls.from_folder's dataset from a record dict, holding device tensors: random_split, HipTubeTrainer.set_data and
    HipTubeSweep.set_data take it as it is (set_data passes device tensors through without a copy)."""
    if cls in (td.ScalarHorizonTubeDataset, td.LevelScalarHorizonTubeDataset):
        w, z, v = build_horizon(records, H_rev, device)
        return cls(w, z, v, H_fwd, H_rev, H_rev + z.shape[-1] + (H_rev + H_fwd) * v.shape[-1] + int(cls.conditioned), H_fwd)
    if cls not in _KIND_OF:
        raise ValueError(f"from_records: {cls.__name__} has no device builder")
    x, y = build_rows(records, _KIND_OF[cls], N, dN, recursive and _KIND_OF[cls] == "scalar", True, mark_last_env, epoch_envs, device)
    return cls(x, y, x.shape[1] + int(cls.conditioned), y.shape[1])


def _cut(ds, s, n):
    """TubeDataset.random_split's two parts for a given offset s and length n (of rows, or of envs for the horizon dataset)."""
    cut = lambda t: (t[s:s + n], torch.vstack((t[:s], t[s + n:])))
    if isinstance(ds, td.ScalarHorizonTubeDataset):
        (w1, w2), (z1, z2), (v1, v2) = cut(ds.w), cut(ds.z), cut(ds.v)
        mk = lambda w, z, v: type(ds)(w, z, v, ds.H_fwd, ds.H_rev, ds.input_dim, ds.output_dim)
        return mk(w1, z1, v1), mk(w2, z2, v2)
    (d1, d2), (t1, t2) = cut(ds.data), cut(ds.target)
    return type(ds)(d1, t1, ds.input_dim, ds.output_dim), type(ds)(d2, t2, ds.input_dim, ds.output_dim)


class SimTubeDataset:
    """A training set that lives on the device with its simulator: the records of the last `resident_epochs` epochs of a HipRomSim
    and the DATASETS[kind] dataset built from them (`.dataset`).  update() -- the training loop's per-epoch hook -- collects
    `refresh` new epochs (one launch each), retires the oldest, rebuilds the rows and sets `changed`; refresh = 0 is a static set.
    Every epoch's last env is dropped, as construct_dataset does to recorded epochs, so a static set equals the one train_tube.py
    --data builds from the same epochs written to disk.

    random_split(p) draws the reference's split once -- a contiguous train piece of int(len p) rows from a drawn offset -- and
    split() reapplies it to the rebuilt rows: the simulator never sets done, so the row count does not change."""

    def __init__(self, sim, kind, N=1, dN=1, recursive=False, H_fwd=50, H_rev=10, T=None, resident_epochs=1, refresh=1):
        if kind not in td.DATASETS:
            raise ValueError(f"kind {kind!r}: one of {sorted(td.DATASETS)}")
        if resident_epochs < 1 or refresh < 0:
            raise ValueError(f"resident_epochs={resident_epochs} must be at least 1 and refresh={refresh} at least 0")
        self.sim, self.kind, self.cls = sim, kind, td.DATASETS[kind]
        self.window = dict(N=N, dN=dN, recursive=recursive, H_fwd=H_fwd, H_rev=H_rev)
        self.T, self.refresh = T, int(refresh)
        self.records = deque(maxlen=int(resident_epochs))
        self.epochs_collected, self.changed, self._split = 0, False, None
        self._collect(int(resident_epochs))
        self._rebuild()

    conditioned = property(lambda self: self.cls.conditioned)
    input_dim = property(lambda self: self.dataset.input_dim)
    output_dim = property(lambda self: self.dataset.output_dim)

    def _collect(self, k):
        for _ in range(k):
            self.records.append(self.sim.collect_epoch(self.T))
            self.epochs_collected += 1

    def raw(self):
        """The resident records, epochs concatenated on the env axis, oldest first."""
        recs = list(self.records)
        return recs[0] if len(recs) == 1 else {k: torch.cat([r[k] for r in recs], dim=0) for k in ("z", "pz_x", "v", "done")}

    def _rebuild(self):
        n = len(self.dataset) if hasattr(self, "dataset") else None
        self.dataset = from_records(self.cls, self.raw(), mark_last_env=True, epoch_envs=self.sim.num_envs, **self.window)
        if n is not None and len(self.dataset) != n:
            raise RuntimeError(f"the rebuilt dataset has {len(self.dataset)} rows, the split was drawn for {n}")

    def __len__(self):
        return len(self.dataset)

    def __getitem__(self, idx):
        return self.dataset[idx]

    def update(self):
        if self.refresh == 0:
            return
        self._collect(self.refresh)
        self._rebuild()
        self.changed = True

    def random_split(self, p):
        n = int(len(self) * p)
        self._split = (int(np.random.randint(len(self) - n)), n)
        return self.split()

    def split(self):
        """(train, test) of the current rows under the split random_split drew."""
        if self._split is None:
            raise RuntimeError("split() before random_split(p)")
        return _cut(self.dataset, *self._split)
