"""Set-pair interaction matrices (include/agbnp_hip.h: agbnp_hip_set_atom_sets, agbnp_hip_num_atom_sets,
agbnp_hip_pair_matrix_host / _device) at the boundaries that need no device: the library exports them under the signatures of the
table, null arguments are refused, the Python wrappers check a partition before they touch the library, and the C++ mirror
compiles against the header."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import AGBNPplugin as TOP
import openmm_agbnp_plugin_amd as P
from openmm_agbnp_plugin_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("agbnp_hip_set_atom_sets", "agbnp_hip_num_atom_sets", "agbnp_hip_pair_matrix_host", "agbnp_hip_pair_matrix_device")


def test_the_entry_points_are_declared_and_exported():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "agbnp_hip.h")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS
        assert f"int {name}(" in header
        getattr(lib, name)
    vp, i, ip, dp = C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_double)
    assert _lib.SIGNATURES["agbnp_hip_set_atom_sets"] == [vp, i, ip, i]
    assert _lib.SIGNATURES["agbnp_hip_num_atom_sets"] == [vp]
    assert _lib.SIGNATURES["agbnp_hip_pair_matrix_host"] == [vp, dp, dp, dp]
    assert _lib.SIGNATURES["agbnp_hip_pair_matrix_device"] == [vp, vp, vp, vp, vp]
    assert "#define AGBNP_HIP_MAX_SETS 2048" in header and _lib.MAX_SETS == 2048
    assert "Not provided: a group form, a binding form, an OpenMM-buffer form" in header
    assert "4 a set-pair interaction matrix" in header  # scalar 20
    names = [lib.agbnp_hip_kernel_name(k).decode() for k in range(lib.agbnp_hip_num_kernels())]
    assert names[-2:] == ["k_decompose", "k_pair_matrix"]


def test_the_python_surface_exists():
    for name in ("set_atom_sets", "num_atom_sets", "pair_matrix", "pair_matrix_device"):
        assert callable(getattr(P.HipCalcAGBNPForceKernel, name))
    assert callable(P.AGBNPContext.getInteractionMatrix)
    assert TOP.HipCalcAGBNPForceKernel is P.HipCalcAGBNPForceKernel and TOP.AGBNPContext is P.AGBNPContext
    assert callable(P.load_sets)


def test_null_arguments_are_invalid():
    lib = _lib.load()
    bad = _lib.ERR_INVALID_ARGUMENT
    sets, pos, matrix, e = np.zeros(1, dtype=np.int32), np.zeros(3), np.zeros(1), C.c_double(0.0)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    assert lib.agbnp_hip_set_atom_sets(None, 1, sets.ctypes.data_as(ip), 1) == bad
    assert lib.agbnp_hip_set_atom_sets(None, 1, None, 1) == bad
    assert lib.agbnp_hip_num_atom_sets(None) == 0
    assert lib.agbnp_hip_pair_matrix_host(None, pos.ctypes.data_as(dp), matrix.ctypes.data_as(dp), C.byref(e)) == bad
    assert lib.agbnp_hip_pair_matrix_host(None, None, None, None) == bad
    assert lib.agbnp_hip_pair_matrix_device(None, None, None, None, None) == bad


class _Fake(P.HipCalcAGBNPForceKernel):
    """A kernel with a handle that must never reach the library."""

    def __init__(self, n):
        super().__init__(device=0)
        self._h = 12345
        self.numParticles = n

    def __del__(self):
        self._h = None


@pytest.fixture()
def no_library(monkeypatch):
    def refuse():
        raise AssertionError("the wrapper reached the library")
    monkeypatch.setattr(_lib, "load", refuse)


@pytest.mark.parametrize("sets, num_sets", [
    ([0, 1, 2], None),              # a wrong length
    ([0, 1, 2, 0, 1], None),
    ([], None),
    ([0, -1, 1, 0], None),          # a negative value
    ([0, 1, 2, 0], 2),              # a value >= num_sets
    ([0, 1, 2, 3], 3),
    ([0, 0, 0, 0], 0),              # num_sets out of 1 .. 2048
    ([0, 0, 0, 0], 2049),
    ([0, 0, 0, 2048], None),
    ([0, 0, 0, 0], -1),
    ([0.5, 0, 0, 0], None),         # not set indices
    ([[0, 0], [0, 0]], None),
    ([0, 0, 0, 2 ** 32], 1),
    (["a", "b", "c", "d"], None),
    (None, None),
])
def test_set_atom_sets_checks_the_partition_first(no_library, sets, num_sets):
    k = _Fake(4)
    with pytest.raises(P.OpenMMException):
        k.set_atom_sets(sets, num_sets)


def test_set_atom_sets_hands_a_good_partition_to_the_library(monkeypatch):
    calls = []

    class Library:
        def agbnp_hip_set_atom_sets(self, handle, n, sets, num_sets):
            calls.append((handle, n, [sets[i] for i in range(n)], num_sets))
            return 0

    monkeypatch.setattr(_lib, "load", Library)
    k = _Fake(5)
    k.set_atom_sets([2, 0, 0, 2, 4])
    k.set_atom_sets(np.array([1, 0, 0, 1, 1], dtype=np.int64), 2048)
    k.set_atom_sets((0, 0, 0, 0, 0))
    assert calls == [(12345, 5, [2, 0, 0, 2, 4], 5), (12345, 5, [1, 0, 0, 1, 1], 2048), (12345, 5, [0, 0, 0, 0, 0], 1)]


def test_an_uninitialised_kernel_refuses(no_library):
    k = P.HipCalcAGBNPForceKernel()
    with pytest.raises(P.OpenMMException):
        k.set_atom_sets([0])
    with pytest.raises(P.OpenMMException):
        k.num_atom_sets()
    with pytest.raises(P.OpenMMException):
        k.pair_matrix(np.zeros((1, 3)))
    with pytest.raises(P.OpenMMException):
        k.pair_matrix_device(1, 2)
    with pytest.raises(P.OpenMMException):
        _Fake(4).pair_matrix(np.zeros((3, 3)))  # a wrong number of positions


def test_the_cpp_mirror_declares_set_atom_sets_and_pair_matrix():
    subprocess.run(["g++", "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-fsyntax-only",
                    os.path.join(ROOT, "tests", "cxx", "TestHipPairMatrix.cpp")], check=True)
