"""Binding-energy evaluations (include/agbnp_hip.h: agbnp_hip_binding_*) at the boundaries that need no device: the library
exports them, agbnp_hip_binding_create refuses a bad ligand list on the host before any device call, the Python class checks its
list before it touches the library, and the C++ mirror compiles against the header."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import AGBNPplugin as TOP
import openmm_agbnp_plugin_amd as P
from openmm_agbnp_plugin_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("agbnp_hip_binding_create", "agbnp_hip_binding_execute_device", "agbnp_hip_binding_energy_device",
       "agbnp_hip_binding_execute_host", "agbnp_hip_binding_energy_host", "agbnp_hip_binding_finish",
       "agbnp_hip_binding_withheld_evaluations", "agbnp_hip_binding_expect_jump", "agbnp_hip_binding_update_parameters",
       "agbnp_hip_binding_set_mode", "agbnp_hip_binding_member", "agbnp_hip_binding_destroy")
N = 6


def test_the_entry_points_are_declared_and_exported():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "agbnp_hip.h")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS
        assert f" {name}(" in header
        getattr(lib, name)
    assert "typedef struct agbnp_hip_binding agbnp_hip_binding;" in header
    assert TOP.BindingEnergy is P.BindingEnergy
    for method in ("execute", "energy", "execute_device", "energy_device", "finish", "withheld", "expect_jump", "set_mode",
                   "copyParametersToContext", "member", "release"):
        assert callable(getattr(P.BindingEnergy, method))
    assert isinstance(P.BindingEnergy.receptor_atoms, property) and isinstance(P.BindingEnergy.ligand_atoms, property)


def test_null_arguments_are_invalid():
    lib = _lib.load()
    bad = _lib.ERR_INVALID_ARGUMENT
    assert lib.agbnp_hip_binding_create(None, 1, None, None, None, None, None, None, 1, 1, 0, 1.0, 0) == bad
    assert lib.agbnp_hip_binding_execute_device(None, None, 0.5, None, None, None, None) == bad
    assert lib.agbnp_hip_binding_energy_device(None, None, 0.5, None, None, None) == bad
    assert lib.agbnp_hip_binding_execute_host(None, None, 0.5, None, None, None) == bad
    assert lib.agbnp_hip_binding_energy_host(None, None, 0.5, None, None) == bad
    assert lib.agbnp_hip_binding_finish(None, None, None) == bad
    assert lib.agbnp_hip_binding_withheld_evaluations(None, None, 0) == -1
    assert lib.agbnp_hip_binding_expect_jump(None) == bad
    assert lib.agbnp_hip_binding_update_parameters(None, 1, None, None, None, None, None) == bad
    assert lib.agbnp_hip_binding_set_mode(None, 0) == bad
    assert lib.agbnp_hip_binding_member(None, 0) is None
    lib.agbnp_hip_binding_destroy(None)


def _create(ligand, version=1, gamma=None, radius=None, method=0):
    lib = _lib.load()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    r = np.full(N, 0.17) if radius is None else np.asarray(radius, dtype=np.float64)
    g = np.full(N, 49.0) if gamma is None else np.asarray(gamma, dtype=np.float64)
    a, q, h = np.full(N, -1.0), np.zeros(N), np.zeros(N, dtype=np.int32)
    lig = np.asarray(ligand, dtype=np.int32)
    handle = C.c_void_p(12345)
    rc = lib.agbnp_hip_binding_create(C.byref(handle), N, r.ctypes.data_as(dp), g.ctypes.data_as(dp), a.ctypes.data_as(dp),
                                      q.ctypes.data_as(dp), h.ctypes.data_as(ip), lig.ctypes.data_as(ip) if len(lig) else ip(C.c_int(0)),
                                      len(lig), version, method, 1.0, 0)
    if rc != _lib.OK:
        assert not handle.value  # a failed create hands no binding out
    else:
        lib.agbnp_hip_binding_destroy(handle)
    return rc, _lib.last_error(None)


@pytest.mark.parametrize("ligand, word", [([0, N], "range"), ([-1], "range"), ([2, 3, 2], "twice"), ([], "1 to N - 1"),
                                           (list(range(N)), "1 to N - 1")])
def test_create_refuses_a_bad_ligand_list_without_a_device(ligand, word):
    rc, msg = _create(ligand)
    assert rc == _lib.ERR_INVALID_ARGUMENT
    assert "agbnp_hip_binding_create" in msg and word in msg


def test_create_checks_its_other_arguments_on_the_host():
    assert _create([1], version=2)[0] == _lib.ERR_INVALID_ARGUMENT
    assert _create([1], version=-1)[0] == _lib.ERR_INVALID_ARGUMENT
    assert _create([1], method=3)[0] == _lib.ERR_INVALID_ARGUMENT
    radius = np.full(N, 0.17)
    radius[4] = 0.0
    assert _create([1], radius=radius)[0] == _lib.ERR_INVALID_ARGUMENT
    gamma = np.full(N, 49.0)
    gamma[3] = 50.0
    rc, msg = _create([1], gamma=gamma)
    assert rc == _lib.ERR_PARAMETERS and "multiple gamma" in msg  # (the reference's message)


@pytest.fixture()
def no_library(monkeypatch):
    def refuse():
        raise AssertionError("the wrapper reached the library")
    monkeypatch.setattr(_lib, "load", refuse)


def test_binding_energy_checks_its_list_first(no_library):
    force = P.AGBNPForce.from_arrays(np.full(N, 0.17), np.full(N, 49.0), np.full(N, -1.0), np.zeros(N), np.zeros(N, dtype=np.int32))
    for ligand in ([], list(range(N)), [0, N], [-1], [2, 2], ["x"], None):
        with pytest.raises(P.OpenMMException):
            P.BindingEnergy(force, ligand)
    with pytest.raises(KeyError):
        P.BindingEnergy(force, [1], mode="no such mode")


def test_the_cpp_mirror_declares_the_binding():
    subprocess.run(["g++", "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-fsyntax-only",
                    os.path.join(ROOT, "tests", "cxx", "TestHipBinding.cpp")], check=True)
