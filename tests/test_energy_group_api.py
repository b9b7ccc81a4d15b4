"""Energy-only replica groups and the jump hint (include/agbnp_hip.h: agbnp_hip_energy_group / _host, agbnp_hip_expect_jump) at
the boundaries that need no device: the library exports them, the Python wrappers check their lists before they touch the
library, the two new scalars are named, and the C++ mirror compiles against the header."""
import os
import re
import subprocess

import numpy as np
import pytest

import AGBNPplugin as TOP
import openmm_agbnp_plugin_amd as P
from openmm_agbnp_plugin_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("agbnp_hip_energy_group", "agbnp_hip_energy_group_host", "agbnp_hip_expect_jump")


def test_the_entry_points_are_declared_and_exported():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "agbnp_hip.h")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS
        assert f"int {name}(" in header
        getattr(lib, name)
    for name in ("energy_group", "energy_group_host"):
        assert callable(getattr(P, name)) and getattr(TOP, name) is getattr(P, name)
    assert callable(P.HipCalcAGBNPForceKernel.expect_jump)


def test_null_arguments_are_invalid():
    lib = _lib.load()
    assert lib.agbnp_hip_energy_group(None, 1, None, None, None) == _lib.ERR_INVALID_ARGUMENT
    assert lib.agbnp_hip_energy_group_host(None, 1, None, None) == _lib.ERR_INVALID_ARGUMENT
    assert lib.agbnp_hip_expect_jump(None) == _lib.ERR_INVALID_ARGUMENT


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


def test_energy_group_checks_its_lists_first(no_library):
    ks = [_Fake(4), _Fake(4)]
    with pytest.raises(P.OpenMMException):
        P.energy_group([], [], [])
    with pytest.raises(P.OpenMMException):
        P.energy_group([_Fake(4) for _ in range(17)], [1] * 17, [1] * 17)
    with pytest.raises(P.OpenMMException):
        P.energy_group(ks, [1], [4, 5])
    with pytest.raises(P.OpenMMException):
        P.energy_group(ks, [1, 2], [5])
    with pytest.raises(P.OpenMMException):
        P.energy_group([ks[0], "not a kernel"], [1, 2], [5, 6])
    with pytest.raises(P.OpenMMException):
        P.energy_group([P.HipCalcAGBNPForceKernel()], [1], [3])  # (never initialised)


def test_energy_group_host_checks_shapes_first(no_library):
    ks = [_Fake(4), _Fake(5)]
    pos = [np.zeros((4, 3)), np.zeros((5, 3))]
    with pytest.raises(P.OpenMMException):
        P.energy_group_host([], [])
    with pytest.raises(P.OpenMMException):
        P.energy_group_host([_Fake(4) for _ in range(17)], [np.zeros((4, 3))] * 17)
    with pytest.raises(P.OpenMMException):
        P.energy_group_host(ks, pos[:1])
    with pytest.raises(P.OpenMMException):
        P.energy_group_host(ks, [np.zeros((5, 3)), np.zeros((5, 3))])
    with pytest.raises(P.OpenMMException):
        P.energy_group_host([ks[0], None], pos)
    with pytest.raises(P.OpenMMException):
        P.energy_group_host([P.HipCalcAGBNPForceKernel()], pos[:1])


def test_expect_jump_needs_an_initialised_kernel(no_library):
    with pytest.raises(P.OpenMMException):
        P.HipCalcAGBNPForceKernel().expect_jump()


def test_scalars_20_and_21_are_named():
    assert P.HipCalcAGBNPForceKernel.SCALARS["last_evaluation_kind"] == 20
    assert P.HipCalcAGBNPForceKernel.SCALARS["group_block_writes"] == 21
    header = open(os.path.join(ROOT, "include", "agbnp_hip.h")).read()
    assert re.search(r"\bAGBNP_HIP_SCALAR_LAST_EVALUATION_KIND = 20,\s*/\* how the last evaluation ENQUEUED", header)
    assert re.search(r"\bAGBNP_HIP_SCALAR_GROUP_BLOCK_WRITES = 21\s*/\* how often the context's group argument blocks", header)


def test_the_cpp_mirror_declares_energy_group_and_expect_jump():
    subprocess.run(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-fsyntax-only",
                    os.path.join(ROOT, "tests", "cxx", "TestHipEnergyGroup.cpp")], check=True)
