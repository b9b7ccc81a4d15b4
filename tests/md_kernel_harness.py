"""What the tests of libagbnp_md.so's kernels share (tests/test_gpu_md_kernels.py, test_gpu_hremd_kernels.py,
test_gpu_fire_kernels.py) and, at the end, what the self-tests of their CPU restatements share.  A plain module, not a
conftest: a test file imports what it uses, the `gpu` fixture included."""
import ctypes as C
import types

import numpy as np
import pytest

# (n, R): one atom, a wave's and a workgroup's edges, a third workgroup with a single atom; one replica, a few, a full group
CASES = [(1, 1), (1, 16), (63, 2), (64, 3), (65, 2), (255, 1), (256, 2), (257, 3), (513, 16)]
_F64 = ("x", "v", "f", "x0", "hdt_m", "mass", "kT", "energy", "acc", "log_pe", "log_ke", "last")
_GUARD = 16  # records of 0xFF in front of and behind a record buffer, which must stay 0xFF
_OWN = object()  # a launch with the device's own argument struct


@pytest.fixture(scope="module")
def gpu(gpu_required):
    torch = pytest.importorskip("torch")
    from openmm_agbnp_plugin_amd import md
    return types.SimpleNamespace(torch=torch, md=md, lib=md._md_lib(), dev=torch.device("cuda:0"))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _up(gpu, a):
    return gpu.torch.from_numpy(np.ascontiguousarray(a).copy()).to(gpu.dev).contiguous()


def _note(worst, key, value):
    worst[key] = max(worst.get(key, 0.0), float(value))


class Part(int):
    """The index of a partial buffer among a launch's arguments."""


class Device:
    """A restatement state as device tensors, and the argument struct over them."""

    def __init__(self, gpu, state):
        self.gpu, self.base = gpu, state
        self.R, self.n = state["x"].shape[:2]
        t = {key: _up(gpu, state[key]) for key in _F64}
        t["seeds"] = _up(gpu, state["seeds"].view(np.int64))
        t["done"] = _up(gpu, state["done"].view(np.int32))
        t["step"] = _up(gpu, state["step"])
        self.t, self.parts = t, [_up(gpu, p) for p in state["parts"]]
        self.g = gpu.md._args(gpu.md._GroupArgs, n=self.n, replicas=self.R, c1=state["c1"], dt=state["dt"], ktether=state["k"],
                              capacity=state["capacity"], **{key: t[key] for key in _F64 + ("seeds", "done", "step")})
        gpu.torch.cuda.synchronize()

    def read(self):
        self.gpu.torch.cuda.synchronize()
        out = {key: val for key, val in self.base.items() if not isinstance(val, (np.ndarray, list))}
        out.update({key: val.cpu().numpy().copy() for key, val in self.t.items()})
        out["seeds"], out["done"] = out["seeds"].view(np.uint64), out["done"].view(np.uint32)
        out["parts"] = [p.cpu().numpy().copy() for p in self.parts]
        return out

    def upload(self, key, a):
        self.t[key].copy_(self.gpu.torch.from_numpy(np.ascontiguousarray(a)))

    def launch(self, name, *args, g=_OWN):
        """One entry point on the current stream, waited for; returns its code."""
        torch = self.gpu.torch
        torch.cuda.synchronize()
        args = [self.parts[a].data_ptr() if isinstance(a, Part) else a for a in args]
        rc = getattr(self.gpu.lib, "agbnp_md_group_" + name)(C.byref(self.g) if g is _OWN else g, *args,
                                                              torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc


def altered(struct, **fields):
    """A reference to a copy of the argument struct with `fields` set."""
    out = type(struct).from_buffer_copy(struct)
    for key, val in fields.items():
        setattr(out, key, val)
    return C.byref(out)


def record_buffer(gpu, state, dtype):
    """state["records"] between guard records on the device, and the log pointer to hand over.  The records of attempt a have
    fixed places in the log that grow with a, and the runs start at a = 2^32 - 3: the pointer is the buffer's address minus
    `record_base` records, so that the places of this run's attempts are the buffer's 0, 1, ...; log_capacity is a log place
    as well, so the kernel refuses every place behind the buffer's share of the log (and forms no address in front of it: the
    places of a run only grow)."""
    guard = np.full(_GUARD * dtype.itemsize, 0xFF, dtype=np.uint8)
    t = _up(gpu, np.concatenate([guard, state["records"].view(np.uint8), guard]))
    return t, (t.data_ptr() + (_GUARD - state["record_base"]) * dtype.itemsize) & 0xFFFFFFFFFFFFFFFF


def split_records(out, dtype):
    """out["records"] as read back from a `record_buffer`: the guards go to out["guards"], the records stay, as `dtype`."""
    raw, size = out["records"], _GUARD * dtype.itemsize
    out["guards"] = np.concatenate([raw[:size], raw[-size:]])
    out["records"] = raw[size:-size].view(dtype).copy()
    return out


# ---- for the self-tests of the restatements (no device)

def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_same_state(a, b, but=()):
    assert a.keys() == b.keys()
    for key in a:
        if key in but:
            continue
        if key == "parts":
            assert all(same_bits(p, q) for p, q in zip(a[key], b[key])), key
        elif isinstance(a[key], np.ndarray):
            assert same_bits(a[key], b[key]), key
        else:
            assert a[key] == b[key], key
