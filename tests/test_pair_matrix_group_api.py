"""Pair-matrix groups and the set-pair matrix of a binding energy (include/agbnp_hip.h: agbnp_hip_pair_matrix_group / _host,
agbnp_hip_binding_set_atom_sets, _num_atom_sets, _pair_matrix_device / _host) at the boundaries that need no device: the library exports them under the signatures of the table, null arguments are refused, the
Python wrappers check partitions, member lists and overlaps before they touch the library, what they hand to the C ABI is pinned
with a recording stand-in (as tests/test_python_marshalling.py does), and the C++ mirror compiles against the header."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import AGBNPplugin as TOP
import openmm_agbnp_plugin_amd as P
from openmm_agbnp_plugin_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("agbnp_hip_pair_matrix_group", "agbnp_hip_pair_matrix_group_host", "agbnp_hip_binding_set_atom_sets",
       "agbnp_hip_binding_num_atom_sets", "agbnp_hip_binding_pair_matrix_device", "agbnp_hip_binding_pair_matrix_host")
DP = C.POINTER(C.c_double)


def test_the_entry_points_are_declared_and_exported():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "agbnp_hip.h")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS
        assert f"int {name}(" in header
        getattr(lib, name)
    vp, i, ip, vpp, dp, dpp = C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_void_p), DP, C.POINTER(DP)
    assert _lib.SIGNATURES["agbnp_hip_pair_matrix_group"] == [vpp, i, vpp, vpp, vpp, vp]
    assert _lib.SIGNATURES["agbnp_hip_pair_matrix_group_host"] == [vpp, i, dpp, dpp, dp]
    assert _lib.SIGNATURES["agbnp_hip_binding_set_atom_sets"] == [vp, i, ip, i]
    assert _lib.SIGNATURES["agbnp_hip_binding_num_atom_sets"] == [vp]
    assert _lib.SIGNATURES["agbnp_hip_binding_pair_matrix_device"] == [vp, vp, vp, vp, vp]
    assert _lib.SIGNATURES["agbnp_hip_binding_pair_matrix_host"] == [vp, dp, dp, dp]
    # the sentence of the single call's documentation stays, and the one behind it names the later additions
    pinned = "Not provided: a group form, a binding form, an OpenMM-buffer form"
    behind = " ".join(header[header.index(pinned):].split("*/")[0].replace("\n *", " ").split())
    assert "agbnp_hip_pair_matrix_group()" in behind and "agbnp_hip_binding_pair_matrix_*()" in behind
    assert "24 S^2 bytes" in header


def test_the_python_surface_exists():
    for name in ("pair_matrix_group", "pair_matrix_group_host"):
        assert callable(getattr(P, name)) and getattr(TOP, name) is getattr(P, name)
    for name in ("set_atom_sets", "num_atom_sets", "pair_matrix", "pair_matrix_device"):
        assert callable(getattr(P.BindingEnergy, name))
    assert TOP.BindingEnergy is P.BindingEnergy


def test_null_arguments_are_invalid():
    lib = _lib.load()
    bad = _lib.ERR_INVALID_ARGUMENT
    assert lib.agbnp_hip_pair_matrix_group(None, 1, None, None, None, None) == bad
    assert lib.agbnp_hip_pair_matrix_group_host(None, 1, None, None, None) == bad
    assert lib.agbnp_hip_binding_set_atom_sets(None, 0, None, 1) == bad
    assert lib.agbnp_hip_binding_num_atom_sets(None) == 0
    assert lib.agbnp_hip_binding_pair_matrix_device(None, None, None, None, None) == bad
    assert lib.agbnp_hip_binding_pair_matrix_host(None, None, None, None) == bad
    # a member count out of range and a null member, refused before any member is looked at
    null = (C.c_void_p * 1)(None)
    for count in (0, -1, 17):
        assert lib.agbnp_hip_pair_matrix_group(null, count, None, None, None, None) == bad
        assert lib.agbnp_hip_pair_matrix_group_host(null, count, None, None, None) == bad
    assert lib.agbnp_hip_pair_matrix_group(null, 1, None, None, None, None) == bad
    assert lib.agbnp_hip_pair_matrix_group_host(null, 1, None, None, None) == bad


class _Fake(P.HipCalcAGBNPForceKernel):
    """A kernel with a handle that must never reach the library, and the partition size set_atom_sets() would have noted."""

    def __init__(self, n, num_sets=0, h=12345):
        super().__init__(device=0)
        self._h = h
        self.numParticles = n
        self._num_sets = num_sets

    def release(self):
        self._h = None


def _fake_binding(n=4, h=0x6000):
    b = P.BindingEnergy.__new__(P.BindingEnergy)
    b._h, b.numParticles = h, n
    b.release = lambda: None
    return b


@pytest.fixture()
def no_library(monkeypatch):
    def refuse():
        raise AssertionError("the wrapper reached the library")
    monkeypatch.setattr(_lib, "load", refuse)


def test_pair_matrix_group_checks_its_lists_first(no_library):
    ks = [_Fake(4, 2), _Fake(4, 3)]
    with pytest.raises(P.OpenMMException, match="1 to 16"):
        P.pair_matrix_group([], [], [])
    with pytest.raises(P.OpenMMException, match="1 to 16"):
        P.pair_matrix_group([_Fake(4, 2) for _ in range(17)], [1] * 17, [1] * 17)
    with pytest.raises(P.OpenMMException):
        P.pair_matrix_group(ks, [1], [4096, 8192])
    with pytest.raises(P.OpenMMException):
        P.pair_matrix_group(ks, [1, 2], [4096])
    with pytest.raises(P.OpenMMException):
        P.pair_matrix_group(ks, [1, 2], [4096, 8192], [7])  # (energy words: none, or one per member)
    with pytest.raises(P.OpenMMException):
        P.pair_matrix_group(ks, None, [4096, 8192])
    with pytest.raises(P.OpenMMException):
        P.pair_matrix_group(ks, [1, 2], None)
    with pytest.raises(P.OpenMMException, match="null pointer"):
        P.pair_matrix_group(ks, [1, 2], [4096, 0])
    with pytest.raises(P.OpenMMException, match="null pointer"):
        P.pair_matrix_group(ks, [1, None], [4096, 8192])
    with pytest.raises(P.OpenMMException):
        P.pair_matrix_group([ks[0], "not a kernel"], [1, 2], [4096, 8192])
    with pytest.raises(P.OpenMMException):
        P.pair_matrix_group([P.HipCalcAGBNPForceKernel()], [1], [4096])  # (never initialised)


def test_pair_matrix_group_checks_partitions_and_overlaps_first(no_library):
    with pytest.raises(P.OpenMMException, match="member 1: no partition has been set"):
        P.pair_matrix_group([_Fake(4, 2), _Fake(4, 0)], [1, 2], [4096, 8192])
    with pytest.raises(P.OpenMMException, match="no partition has been set"):
        P.pair_matrix_group_host([_Fake(4, 0)], [np.zeros((4, 3))])
    ks = [_Fake(4, 2), _Fake(4, 3)]  # matrices of 4 and 9 doubles: 32 and 72 bytes
    with pytest.raises(P.OpenMMException, match="matrices of two members overlap"):
        P.pair_matrix_group(ks, [1, 2], [4096, 4096 + 24])           # member 1 begins in member 0's last word
    with pytest.raises(P.OpenMMException, match="matrices of two members overlap"):
        P.pair_matrix_group(ks, [1, 2], [4096 + 64, 4096])           # member 0 begins in member 1's last word
    with pytest.raises(P.OpenMMException, match="matrices of two members overlap"):
        P.pair_matrix_group(ks, [1, 2], [4096, 8192], [8192 + 64, 16384])  # member 0's energy word inside member 1's matrix
    with pytest.raises(P.OpenMMException, match="matrices of two members overlap"):
        P.pair_matrix_group(ks, [1, 2], [4096, 8192], [4096 + 24, 16384])  # a member's energy word inside its own matrix
    with pytest.raises(P.OpenMMException, match="energy words of two members overlap"):
        P.pair_matrix_group(ks, [1, 2], [4096, 8192], [16384, 16384])


def test_pair_matrix_group_host_checks_shapes_first(no_library):
    ks = [_Fake(4, 2), _Fake(5, 2)]
    pos = [np.zeros((4, 3)), np.zeros((5, 3))]
    with pytest.raises(P.OpenMMException):
        P.pair_matrix_group_host([], [])
    with pytest.raises(P.OpenMMException):
        P.pair_matrix_group_host([_Fake(4, 2) for _ in range(17)], [np.zeros((4, 3))] * 17)
    with pytest.raises(P.OpenMMException):
        P.pair_matrix_group_host(ks, pos[:1])
    with pytest.raises(P.OpenMMException):
        P.pair_matrix_group_host(ks, [np.zeros((5, 3)), np.zeros((5, 3))])
    with pytest.raises(P.OpenMMException):
        P.pair_matrix_group_host([ks[0], None], pos)
    with pytest.raises(P.OpenMMException):
        P.pair_matrix_group_host([P.HipCalcAGBNPForceKernel()], pos[:1])


def test_a_binding_checks_its_partition_first(no_library):
    b = _fake_binding(4)
    for sets, num_sets in (([0, 1, 2], None),            # one index too few
                           ([0, 1, 2, 3, 0], None),       # one too many
                           ([0, 1, -1, 0], None),         # a negative index
                           ([0, 1, 2, 3], 3),             # an index beyond num_sets - 1
                           ([0.5, 1, 2, 3], None),        # not an integer
                           ([[0, 1], [2, 3]], None),      # not a list
                           ([0, 1, 2, 3], 0),             # num_sets out of range
                           ([0, 1, 2, 3], _lib.MAX_SETS + 1),
                           ("abcd", None)):
        with pytest.raises(P.OpenMMException, match="set_atom_sets"):
            b.set_atom_sets(sets, num_sets)


def test_a_released_binding_refuses_the_matrix_calls(no_library):
    b = P.BindingEnergy.__new__(P.BindingEnergy)  # (no handle: what release() leaves)
    b.numParticles = 4
    with pytest.raises(P.OpenMMException, match="released"):
        b.set_atom_sets([0, 0, 1, 1])
    with pytest.raises(P.OpenMMException, match="released"):
        b.num_atom_sets()
    with pytest.raises(P.OpenMMException, match="released"):
        b.pair_matrix(np.zeros((4, 3)))
    with pytest.raises(P.OpenMMException, match="released"):
        b.pair_matrix_device(1, 2)


# ---- what crosses the C ABI ------------------------------------------------------------------------------------------------------
class Recorder:
    """Stands for the library: every agbnp_* attribute records (symbol, arguments) and returns `fail[symbol]` (0)."""

    def __init__(self):
        self.calls, self.fail, self.sets = [], {}, 3

    def __getattr__(self, name):
        if not name.startswith("agbnp_"):
            raise AttributeError(name)

        def call(*args):
            self.calls.append((name, args))
            if name == "agbnp_hip_last_error":
                return b"recorded failure for handle %#x" % address(args[0])
            if name.endswith("num_atom_sets"):
                return self.sets
            for a in args:  # output arguments passed with byref
                out = getattr(a, "_obj", None)
                if isinstance(out, C.c_double):
                    out.value = 10.5
            return self.fail.get(name, 0)
        return call


def address(a):
    """An argument as the integer the callee would see: None, 0 and a NULL pointer are all 0."""
    if a is None:
        return 0
    if isinstance(a, C.c_void_p):
        return a.value or 0
    if isinstance(a, C._Pointer):
        return C.cast(a, C.c_void_p).value or 0
    assert type(a) is int, a
    return a


@pytest.fixture()
def rec(monkeypatch):
    r = Recorder()
    monkeypatch.setattr(_lib, "load", lambda: r)
    return r


def test_pair_matrix_group_marshals_one_pointer_per_member(rec):
    ks = [_Fake(4, 2, 0x5000), _Fake(5, 3, 0x5100)]
    P.pair_matrix_group(ks, [0x100, 0x100], [0x1000, 0x2000], [0x3000, 0x3008], stream=0x77)  # (shared positions are fine)
    (name, args), = rec.calls
    assert name == "agbnp_hip_pair_matrix_group" and len(args) == 6
    hs, count, pos, mats, ene, stream = args
    assert count == 2 and address(stream) == 0x77
    assert [hs[0], hs[1]] == [0x5000, 0x5100]
    assert [pos[0], pos[1]] == [0x100, 0x100] and [mats[0], mats[1]] == [0x1000, 0x2000] and [ene[0], ene[1]] == [0x3000, 0x3008]
    rec.calls.clear()
    P.pair_matrix_group(ks, [0x100, 0x200], [0x1000, 0x2000])  # no energy words, no stream: NULL and NULL
    (name, args), = rec.calls
    assert args[4] is None and address(args[5]) == 0
    rec.calls.clear()
    rec.fail["agbnp_hip_pair_matrix_group"] = _lib.ERR_INVALID_ARGUMENT
    with pytest.raises(P.OpenMMException, match="handle 0x5000"):  # (the first member's message)
        P.pair_matrix_group(ks, [0x100, 0x200], [0x1000, 0x2000])


def test_pair_matrix_group_host_marshals_and_returns_the_members_matrices(rec):
    ks = [_Fake(4, 2, 0x5000), _Fake(5, 3, 0x5100)]
    positions = [np.arange(12.0).reshape(4, 3), np.arange(15.0).reshape(5, 3)]
    energies, matrices = P.pair_matrix_group_host(ks, positions)
    (name, args), = rec.calls
    assert name == "agbnp_hip_pair_matrix_group_host" and len(args) == 5
    hs, count, pos, mats, ene = args
    assert count == 2 and [hs[0], hs[1]] == [0x5000, 0x5100]
    assert [pos[m][k] for m in range(2) for k in (0, 11)] == [0.0, 11.0, 0.0, 11.0]
    assert [m.shape for m in matrices] == [(2, 2), (3, 3)] and all(m.dtype == np.float64 and m.flags.c_contiguous for m in matrices)
    assert [address(mats[m]) for m in range(2)] == [m.ctypes.data for m in matrices]
    assert isinstance(ene, DP) and energies == [0.0, 0.0]
    rec.fail["agbnp_hip_pair_matrix_group_host"] = _lib.ERR_DEVICE
    with pytest.raises(P.OpenMMException, match="handle 0x5000"):
        P.pair_matrix_group_host(ks, positions)


def test_the_binding_calls_marshal(rec):
    b = _fake_binding(4, 0x6000)
    b.set_atom_sets([2, 0, 0, 1])
    (name, args), = rec.calls
    assert name == "agbnp_hip_binding_set_atom_sets" and len(args) == 4
    assert args[0] == 0x6000 and args[1] == 4 and [args[2][k] for k in range(4)] == [2, 0, 0, 1] and args[3] == 3
    assert isinstance(args[2], C.POINTER(C.c_int))
    rec.calls.clear()
    b.set_atom_sets([0, 0, 0, 1], num_sets=7)  # (empty sets are allowed)
    assert rec.calls[0][1][3] == 7
    rec.calls.clear()
    assert b.num_atom_sets() == 3 and rec.calls == [("agbnp_hip_binding_num_atom_sets", (0x6000,))]
    rec.calls.clear()
    d, u = b.pair_matrix(np.arange(12.0).reshape(4, 3))
    name, args = rec.calls[-1]
    assert name == "agbnp_hip_binding_pair_matrix_host" and len(args) == 4 and args[0] == 0x6000
    assert args[1][11] == 11.0 and address(args[2]) == d.ctypes.data and d.shape == (3, 3) and u == 10.5
    rec.calls.clear()
    b.pair_matrix_device(0x100, 0x200, None, 0x77)
    assert [(n, [address(x) for x in a]) for n, a in rec.calls] == [("agbnp_hip_binding_pair_matrix_device", [0x6000, 0x100, 0x200, 0, 0x77])]
    rec.calls.clear()
    b.pair_matrix_device(0x100, 0x200, 0x300)
    assert [address(x) for x in rec.calls[0][1]] == [0x6000, 0x100, 0x200, 0x300, 0]
    rec.fail["agbnp_hip_binding_pair_matrix_device"] = _lib.ERR_INVALID_ARGUMENT
    with pytest.raises(P.OpenMMException, match="handle 0x0"):  # (a binding's messages are the thread's, not a handle's)
        b.pair_matrix_device(0x100, 0x200)
    rec.fail["agbnp_hip_binding_set_atom_sets"] = _lib.ERR_DEVICE
    with pytest.raises(P.OpenMMException):
        b.set_atom_sets([0, 0, 0, 0])


def test_a_member_view_knows_the_bindings_partition(rec):
    b = _fake_binding(4, 0x6000)
    b._device, b._mode = 0, 0
    b._receptor, b._ligand = np.arange(3), np.arange(3, 4)
    assert b.member(0)._num_sets == 0
    b.set_atom_sets([0, 1, 1, 0])
    views = [b.member(m) for m in range(3)]
    assert [v._num_sets for v in views] == [2, 2, 2]
    for v in views:
        v.release()


def test_the_cpp_mirror_declares_the_group_and_the_binding_matrix():
    subprocess.run(["g++", "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-fsyntax-only",
                    os.path.join(ROOT, "tests", "cxx", "TestHipPairMatrixGroup.cpp")], check=True)
