"""Energy-only evaluations (include/agbnp_hip.h: agbnp_hip_energy_host / _device / _openmm) at the boundaries that need no
device: the library exports them, null arguments are refused, the Python kernel fails the OpenMM way without a device, and the
OpenMM glue that routes includeForces = false through them still compiles against the test double of the OpenMM API."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import openmm_agbnp_plugin_amd as P
from openmm_agbnp_plugin_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("agbnp_hip_energy_host", "agbnp_hip_energy_device", "agbnp_hip_energy_openmm")


def test_the_energy_only_entry_points_are_exported():
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.SYMBOLS
        getattr(lib, name)
    header = open(os.path.join(ROOT, "include", "agbnp_hip.h")).read()
    for name in NEW:
        assert f"int {name}(" in header


def test_a_null_context_is_an_invalid_argument():
    lib = _lib.load()
    e = C.c_double(0.0)
    pos = np.zeros(3)
    assert lib.agbnp_hip_energy_host(None, pos.ctypes.data_as(C.POINTER(C.c_double)), C.byref(e)) == _lib.ERR_INVALID_ARGUMENT
    assert lib.agbnp_hip_energy_device(None, None, None, None) == _lib.ERR_INVALID_ARGUMENT
    assert lib.agbnp_hip_energy_openmm(None, None, 1, None, None, 8, None, 1, 0, None) == _lib.ERR_INVALID_ARGUMENT


def test_a_null_energy_pointer_is_an_invalid_argument():
    """A context is needed to get past the null-context check; without a device there is none, and the same calls with a
    context are covered on the GPU box (tests/test_gpu_energy_only.py)."""
    lib = _lib.load()
    if lib.agbnp_hip_device_count() == 0:
        assert lib.agbnp_hip_energy_host(None, None, None) == _lib.ERR_INVALID_ARGUMENT
        return
    s = P.load_system("fixture264")
    k = P.HipCalcAGBNPForceKernel(device=0)
    k.initialize(P.AGBNPForce.from_arrays(*s.params(), version=1))
    pos = np.ascontiguousarray(s.pos, dtype=np.float64)
    dp = pos.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.agbnp_hip_energy_host(k._h, dp, None) == _lib.ERR_INVALID_ARGUMENT
    assert lib.agbnp_hip_energy_device(k._h, C.c_void_p(pos.ctypes.data), None, None) == _lib.ERR_INVALID_ARGUMENT
    assert lib.agbnp_hip_energy_openmm(k._h, C.c_void_p(pos.ctypes.data), 1, None, None, s.n, None, 1, 0, None) == _lib.ERR_INVALID_ARGUMENT
    assert "null pointer" in _lib.last_error(k._h)


def test_energy_without_a_device_fails_with_an_openmm_exception():
    """Without a device, initialize() and energy() raise OpenMMException; with one, energy() on a kernel that was never
    initialised does."""
    s = P.load_system("fixture264")
    if _lib.load().agbnp_hip_device_count() > 0:
        with pytest.raises(P.OpenMMException):
            P.HipCalcAGBNPForceKernel(device=0).energy(s.pos)
        return
    k = P.HipCalcAGBNPForceKernel(device=0)
    with pytest.raises(P.OpenMMException):
        k.initialize(P.AGBNPForce.from_arrays(*s.params(), version=1))
    with pytest.raises(P.OpenMMException):
        k.energy(s.pos)
    ctx_force = P.AGBNPForce.from_arrays(*s.params(), version=1)
    with pytest.raises(P.OpenMMException):
        P.AGBNPContext(ctx_force, device=0).getEnergy()


def test_the_glue_compiles_with_the_energy_only_path():
    mock = os.path.join(ROOT, "tests", "openmm_mock")
    common = ["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{mock}", f"-I{ROOT}/include",
              f"-I{ROOT}/openmm_glue", f"-I{mock}/agbnp_api", "-fsyntax-only", "-Wall"]
    subprocess.run(common + [os.path.join(ROOT, "openmm_glue", "HipAGBNPKernels.cpp")], check=True)
    subprocess.run(common + [os.path.join(ROOT, "tests", "cxx", "TestHipPlatformEnergyOnly.cpp")], check=True)
    glue = open(os.path.join(ROOT, "openmm_glue", "HipAGBNPKernels.cpp")).read()
    assert "agbnp_hip_energy_openmm(" in glue


def test_the_cpp_mirror_declares_energy():
    subprocess.run(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-fsyntax-only", "-x", "c++", "-"],
                   input='#include "%s"\ndouble (AGBNPPlugin::HipCalcAGBNPForceKernel::*p)(const std::vector<double>&) = '
                         '&AGBNPPlugin::HipCalcAGBNPForceKernel::energy;\n' % os.path.join(ROOT, "cpp", "AGBNPForce.h"),
                   text=True, check=True)
