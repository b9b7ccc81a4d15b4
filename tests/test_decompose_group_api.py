"""Decomposition groups and the per-atom decomposition of a binding energy (include/agbnp_hip.h: agbnp_hip_decompose_group /
_host, agbnp_hip_binding_decompose_device / _host) at the boundaries that need no device: the library exports them under the
signatures of the table, null arguments are refused, the Python wrappers check their lists before they touch the library, and
the C++ mirror compiles against the header."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import AGBNPplugin as TOP
import openmm_agbnp_plugin_amd as P
from openmm_agbnp_plugin_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("agbnp_hip_decompose_group", "agbnp_hip_decompose_group_host", "agbnp_hip_binding_decompose_device",
       "agbnp_hip_binding_decompose_host")


def test_the_entry_points_are_declared_and_exported():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "agbnp_hip.h")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS
        assert f"int {name}(" in header
        getattr(lib, name)
    vp, i, vpp, dp, dpp = C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_double), C.POINTER(C.POINTER(C.c_double))
    assert _lib.SIGNATURES["agbnp_hip_decompose_group"] == [vpp, i, vpp, vpp, vpp, vp]
    assert _lib.SIGNATURES["agbnp_hip_decompose_group_host"] == [vpp, i, dpp, dpp, dp]
    assert _lib.SIGNATURES["agbnp_hip_binding_decompose_device"] == [vp, vp, vp, vp, vp]
    assert _lib.SIGNATURES["agbnp_hip_binding_decompose_host"] == [vp, dp, dp, dp]
    assert "no group form" not in header


def test_the_python_surface_exists():
    for name in ("decompose_group", "decompose_group_host"):
        assert callable(getattr(P, name)) and getattr(TOP, name) is getattr(P, name)
    assert TOP.BindingEnergy is P.BindingEnergy
    assert callable(P.BindingEnergy.decompose) and callable(P.BindingEnergy.decompose_device)


def test_null_arguments_are_invalid():
    lib = _lib.load()
    bad = _lib.ERR_INVALID_ARGUMENT
    assert lib.agbnp_hip_decompose_group(None, 1, None, None, None, None) == bad
    assert lib.agbnp_hip_decompose_group_host(None, 1, None, None, None) == bad
    assert lib.agbnp_hip_binding_decompose_device(None, None, None, None, None) == bad
    assert lib.agbnp_hip_binding_decompose_host(None, None, None, None) == bad
    # a member count out of range and a null member, refused before any member is looked at
    null = (C.c_void_p * 1)(None)
    for count in (0, -1, 17):
        assert lib.agbnp_hip_decompose_group(null, count, None, None, None, None) == bad
        assert lib.agbnp_hip_decompose_group_host(null, count, None, None, None) == bad
    assert lib.agbnp_hip_decompose_group(null, 1, None, None, None, None) == bad
    assert lib.agbnp_hip_decompose_group_host(null, 1, None, None, None) == bad


class _Fake(P.HipCalcAGBNPForceKernel):
    """A kernel with a handle that must never reach the library."""

    def __init__(self, n):
        super().__init__(device=0)
        self._h = 12345
        self.numParticles = n


@pytest.fixture()
def no_library(monkeypatch):
    def refuse():
        raise AssertionError("the wrapper reached the library")
    monkeypatch.setattr(_lib, "load", refuse)


def test_decompose_group_checks_its_lists_first(no_library):
    ks = [_Fake(4), _Fake(4)]
    with pytest.raises(P.OpenMMException):
        P.decompose_group([], [], [])
    with pytest.raises(P.OpenMMException):
        P.decompose_group([_Fake(4) for _ in range(17)], [1] * 17, [1] * 17)
    with pytest.raises(P.OpenMMException):
        P.decompose_group(ks, [1], [4, 5])
    with pytest.raises(P.OpenMMException):
        P.decompose_group(ks, [1, 2], [5])
    with pytest.raises(P.OpenMMException):
        P.decompose_group(ks, [1, 2], [5, 6], [7])  # (energy words: none, or one per member)
    with pytest.raises(P.OpenMMException):
        P.decompose_group(ks, None, [5, 6])
    with pytest.raises(P.OpenMMException):
        P.decompose_group(ks, [1, 2], None)
    with pytest.raises(P.OpenMMException):
        P.decompose_group([ks[0], "not a kernel"], [1, 2], [5, 6])
    with pytest.raises(P.OpenMMException):
        P.decompose_group([P.HipCalcAGBNPForceKernel()], [1], [3])  # (never initialised)


def test_decompose_group_host_checks_shapes_first(no_library):
    ks = [_Fake(4), _Fake(5)]
    pos = [np.zeros((4, 3)), np.zeros((5, 3))]
    with pytest.raises(P.OpenMMException):
        P.decompose_group_host([], [])
    with pytest.raises(P.OpenMMException):
        P.decompose_group_host([_Fake(4) for _ in range(17)], [np.zeros((4, 3))] * 17)
    with pytest.raises(P.OpenMMException):
        P.decompose_group_host(ks, pos[:1])
    with pytest.raises(P.OpenMMException):
        P.decompose_group_host(ks, [np.zeros((5, 3)), np.zeros((5, 3))])
    with pytest.raises(P.OpenMMException):
        P.decompose_group_host([ks[0], None], pos)
    with pytest.raises(P.OpenMMException):
        P.decompose_group_host([P.HipCalcAGBNPForceKernel()], pos[:1])


def test_a_released_binding_refuses_to_decompose(no_library):
    b = P.BindingEnergy.__new__(P.BindingEnergy)  # (no handle: what release() leaves)
    b.numParticles = 4
    with pytest.raises(P.OpenMMException):
        b.decompose(np.zeros((4, 3)))
    with pytest.raises(P.OpenMMException):
        b.decompose_device(1, 2)


def test_the_cpp_mirror_declares_decompose_group_and_the_binding_decomposition():
    subprocess.run(["g++", "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-fsyntax-only",
                    os.path.join(ROOT, "tests", "cxx", "TestHipBindingDecomposition.cpp")], check=True)
