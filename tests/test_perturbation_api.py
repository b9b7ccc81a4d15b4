"""Perturbation energies (include/agbnp_hip.h: agbnp_hip_set_parameter_sets, agbnp_hip_num_parameter_sets,
agbnp_hip_perturbed_energies_host / _device / _group / _group_host) at the boundaries that need no device: the library exports
them under the signatures of the table, null arguments are refused, the Python wrappers check the sets before they touch the
library, and the C++ mirror compiles against the header."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import AGBNPplugin as TOP
import openmm_agbnp_plugin_amd as P
from openmm_agbnp_plugin_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z = np.zeros
NEW = ("agbnp_hip_set_parameter_sets", "agbnp_hip_num_parameter_sets", "agbnp_hip_perturbed_energies_host",
       "agbnp_hip_perturbed_energies_device", "agbnp_hip_perturbed_energies_group", "agbnp_hip_perturbed_energies_group_host")


def test_the_entry_points_are_declared_and_exported():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "agbnp_hip.h")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS
        assert f"int {name}(" in header
        getattr(lib, name)
    vp, i, dp = C.c_void_p, C.c_int, C.POINTER(C.c_double)
    vpp, dpp = C.POINTER(C.c_void_p), C.POINTER(dp)
    assert _lib.SIGNATURES["agbnp_hip_set_parameter_sets"] == [vp, i, i, dp, dp, dp]
    assert _lib.SIGNATURES["agbnp_hip_num_parameter_sets"] == [vp]
    assert _lib.SIGNATURES["agbnp_hip_perturbed_energies_host"] == [vp, dp, dp, dp]
    assert _lib.SIGNATURES["agbnp_hip_perturbed_energies_device"] == [vp, vp, vp, vp, vp]
    assert _lib.SIGNATURES["agbnp_hip_perturbed_energies_group"] == [vpp, i, vpp, vpp, vpp, vp]
    assert _lib.SIGNATURES["agbnp_hip_perturbed_energies_group_host"] == [vpp, i, dpp, dpp, dp]
    assert "#define AGBNP_HIP_MAX_PARAMETER_SETS 16" in header and _lib.MAX_PARAMETER_SETS == 16
    assert "5 perturbation energies" in header  # scalar 20
    assert "Not provided: forces under the other sets, a binding form, an OpenMM-buffer form" in header
    # the launch has no entry of its own in the profiling table: the table ends as it did
    names = [lib.agbnp_hip_kernel_name(k).decode() for k in range(lib.agbnp_hip_num_kernels())]
    assert names[-2:] == ["k_decompose", "k_pair_matrix"] and "k_perturb" not in names


def test_the_build_id_covers_the_new_kernel_file():
    makefile = open(os.path.join(ROOT, "openmm_agbnp_plugin_amd", "csrc", "Makefile")).read()
    sources = [line for line in makefile.splitlines() if line.startswith("SRC =")][0].split()
    assert "perturb_kernels.hip" in sources
    assert "cat $(SRC) " in makefile  # (SRC_HASH: every source enters the id)


def test_the_python_surface_exists():
    for name in ("set_parameter_sets", "num_parameter_sets", "perturbed_energies", "perturbed_energies_device"):
        assert callable(getattr(P.HipCalcAGBNPForceKernel, name))
    assert callable(P.AGBNPContext.getPerturbedEnergies)
    assert callable(P.perturbed_energies_group) and callable(P.perturbed_energies_group_host)
    assert TOP.perturbed_energies_group is P.perturbed_energies_group
    assert TOP.perturbed_energies_group_host is P.perturbed_energies_group_host
    assert TOP.HipCalcAGBNPForceKernel is P.HipCalcAGBNPForceKernel


def test_null_arguments_are_invalid():
    lib = _lib.load()
    bad = _lib.ERR_INVALID_ARGUMENT
    x, e = np.zeros(3), C.c_double(0.0)
    dp = C.POINTER(C.c_double)
    xp = x.ctypes.data_as(dp)
    assert lib.agbnp_hip_set_parameter_sets(None, 1, 1, xp, xp, xp) == bad
    assert lib.agbnp_hip_set_parameter_sets(None, 1, 1, None, None, None) == bad
    assert lib.agbnp_hip_num_parameter_sets(None) == 0
    assert lib.agbnp_hip_perturbed_energies_host(None, xp, xp, C.byref(e)) == bad
    assert lib.agbnp_hip_perturbed_energies_host(None, None, None, None) == bad
    assert lib.agbnp_hip_perturbed_energies_device(None, None, None, None, None) == bad
    assert lib.agbnp_hip_perturbed_energies_group(None, 1, None, None, None, None) == bad
    assert lib.agbnp_hip_perturbed_energies_group_host(None, 1, None, None, None) == bad
    null = (C.c_void_p * 1)(None)
    assert lib.agbnp_hip_perturbed_energies_group(null, 1, None, None, None, None) == bad
    assert lib.agbnp_hip_perturbed_energies_group(null, 0, None, None, None, None) == bad
    assert lib.agbnp_hip_perturbed_energies_group(null, 17, None, None, None, None) == bad


class _Fake(P.HipCalcAGBNPForceKernel):
    """A kernel with a handle that must never reach the library."""

    def __init__(self, n, sets=0):
        super().__init__(device=0)
        self._h = 12345
        self.numParticles = n
        self._num_parameter_sets = sets

    def __del__(self):
        self._h = None


@pytest.fixture()
def no_library(monkeypatch):
    def refuse():
        raise AssertionError("the wrapper reached the library")
    monkeypatch.setattr(_lib, "load", refuse)


@pytest.mark.parametrize("gamma, alpha, charge", [
    (Z(3), Z(4), Z(4)),                      # a wrong length
    (Z((2, 4)), Z((2, 3)), Z((2, 4))),
    (Z((2, 4)), Z((3, 4)), Z((2, 4))),       # different numbers of sets
    (Z(4), Z((2, 4)), Z((2, 4))),
    (Z((0, 4)), Z((0, 4)), Z((0, 4))),       # M out of 1 .. 16
    (Z((17, 4)), Z((17, 4)), Z((17, 4))),
    (Z((1, 2, 4)), Z((1, 2, 4)), Z((1, 2, 4))),  # not [M, N]
    (Z(()), Z(()), Z(())),
    (np.full(4, np.nan), Z(4), Z(4)),        # not finite
    (Z(4), Z(4), np.full(4, np.inf)),
    (["a", "b", "c", "d"], Z(4), Z(4)),      # not numbers
    (None, Z(4), Z(4)),
    (Z(4), [[0, 1], [2]], Z(4)),
])
def test_set_parameter_sets_checks_the_shapes_first(no_library, gamma, alpha, charge):
    k = _Fake(4)
    with pytest.raises(P.OpenMMException):
        k.set_parameter_sets(gamma, alpha, charge)
    assert k._num_parameter_sets == 0


def test_set_parameter_sets_hands_good_sets_to_the_library(monkeypatch):
    calls = []

    class Library:
        def agbnp_hip_set_parameter_sets(self, handle, n, m, gamma, alpha, charge):
            calls.append((handle, n, m, [gamma[i] for i in range(n * m)], [alpha[i] for i in range(n * m)], [charge[i] for i in range(n * m)]))
            return 0

    monkeypatch.setattr(_lib, "load", Library)
    k = _Fake(2)
    k.set_parameter_sets([1, 2], [3, 4], [5, 6])  # one set as [N]
    assert k._num_parameter_sets == 1
    k.set_parameter_sets([[1, 2], [3, 4]], np.array([[5, 6], [7, 8]], dtype=np.float32), np.array([[9, 10], [11, 12]])[:, ::-1])
    assert k._num_parameter_sets == 2
    assert calls == [(12345, 2, 1, [1.0, 2.0], [3.0, 4.0], [5.0, 6.0]),
                     (12345, 2, 2, [1.0, 2.0, 3.0, 4.0], [5.0, 6.0, 7.0, 8.0], [10.0, 9.0, 12.0, 11.0])]


def test_an_uninitialised_kernel_refuses(no_library):
    k = P.HipCalcAGBNPForceKernel()
    with pytest.raises(P.OpenMMException):
        k.set_parameter_sets([0.0], [0.0], [0.0])
    with pytest.raises(P.OpenMMException):
        k.num_parameter_sets()
    with pytest.raises(P.OpenMMException):
        k.perturbed_energies(np.zeros((1, 3)))
    with pytest.raises(P.OpenMMException):
        k.perturbed_energies_device(1, 2)
    with pytest.raises(P.OpenMMException):
        _Fake(4, 2).perturbed_energies(np.zeros((3, 3)))  # a wrong number of positions


def test_the_group_wrappers_check_their_members_first(no_library):
    a, b, bare = _Fake(4, 2), _Fake(4, 3), _Fake(4, 0)
    with pytest.raises(P.OpenMMException, match="1 to 16"):
        P.perturbed_energies_group([], [], [])
    with pytest.raises(P.OpenMMException, match="1 to 16"):
        P.perturbed_energies_group([_Fake(4, 1) for _ in range(17)], [1] * 17, [1] * 17)
    with pytest.raises(P.OpenMMException, match="member 1: no parameter sets have been set"):
        P.perturbed_energies_group([a, bare], [1, 2], [3, 4])
    with pytest.raises(P.OpenMMException, match="member 0: no parameter sets have been set"):
        P.perturbed_energies_group_host([bare], [np.zeros((4, 3))])
    with pytest.raises(P.OpenMMException, match="entries"):
        P.perturbed_energies_group([a, b], [1, 2], [3])
    with pytest.raises(P.OpenMMException, match="entries"):
        P.perturbed_energies_group([a, b], [1, 2], [3, 4], [5])
    with pytest.raises(P.OpenMMException, match="needed"):
        P.perturbed_energies_group([a, b], [1, 2], None)
    with pytest.raises(P.OpenMMException, match="positions"):
        P.perturbed_energies_group_host([a, b], [np.zeros((4, 3))])
    with pytest.raises(P.OpenMMException, match="positions"):
        P.perturbed_energies_group_host([a, b], [np.zeros((4, 3)), np.zeros((3, 3))])
    with pytest.raises(P.OpenMMException):
        P.perturbed_energies_group([a, object()], [1, 2], [3, 4])


def test_the_group_marshalling_is_the_other_kinds(monkeypatch):
    """One pointer per member and list, NULL for a missing own-energy list; the host form hands out [M_i] arrays, M_i the
    library's count -- not the wrapper's, which another wrapper of the same handle may have left behind."""
    calls = []

    class Library:
        def agbnp_hip_perturbed_energies_group(self, handles, count, pos, ene, own, stream):
            calls.append(("device", list(handles), count, list(pos), list(ene), own if own is None else list(own), stream.value))
            return 0

        def agbnp_hip_num_parameter_sets(self, handle):  # (the host form sizes its arrays by the library's count)
            return {111: 2, 222: 3}[handle]

        def agbnp_hip_perturbed_energies_group_host(self, handles, count, pos, ene, own):
            for i in range(count):
                own[i] = 10.0 + i
            ene[0][1] = 7.0
            ene[1][2] = 8.0
            calls.append(("host", list(handles), count))
            return 0

    monkeypatch.setattr(_lib, "load", Library)
    a, b = _Fake(4, 2), _Fake(4, 3)
    a._h, b._h = 111, 222
    P.perturbed_energies_group([a, b], [1, 2], [3, 4], None, 9)
    P.perturbed_energies_group([a, b], [1, 2], [3, 4], [5, 6])
    assert calls[0] == ("device", [111, 222], 2, [1, 2], [3, 4], None, 9)
    assert calls[1] == ("device", [111, 222], 2, [1, 2], [3, 4], [5, 6], None)
    a._num_parameter_sets = 1  # (stale: sets of another size were set through another wrapper of the handle)
    own, energies = P.perturbed_energies_group_host([a, b], [np.zeros((4, 3)), np.zeros((4, 3))])
    assert own == [10.0, 11.0] and [e.shape for e in energies] == [(2,), (3,)]
    assert energies[0][1] == 7.0 and energies[1][2] == 8.0
    assert calls[2] == ("host", [111, 222], 2)


def test_the_cpp_mirror_declares_the_perturbation_calls():
    program = """#include "%s"
using K = AGBNPPlugin::HipCalcAGBNPForceKernel;
void (K::*set)(const std::vector<double>&, const std::vector<double>&, const std::vector<double>&) = &K::setParameterSets;
int (K::*count)() const = &K::numParameterSets;
double (K::*one)(const std::vector<double>&, std::vector<double>&) = &K::perturbedEnergies;
std::vector<double> (*group)(const std::vector<K*>&, const std::vector<std::vector<double>>&, std::vector<std::vector<double>>&) =
    &K::perturbedEnergiesGroup;
static_assert(AGBNP_HIP_MAX_PARAMETER_SETS == 16, "");
""" % os.path.join(ROOT, "cpp", "AGBNPForce.h")
    subprocess.run(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-fsyntax-only", "-Wall", "-x", "c++", "-"],
                   input=program, text=True, check=True)
