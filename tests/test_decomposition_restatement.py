"""Per-atom decomposition (include/agbnp_hip.h: agbnp_hip_decompose_host / _device) at the boundaries that need no device.

The identities: the four planes of tests/decomposition_restatement.py -- built from the oracle's self volumes and Born radii --
sum to the energy Oracle.execute() returns, and their partial sums are the oracle's own components E_vol1 + E_vol2, E_vdw and
E_gb, within SAME (1e-9 kJ/mol, tests/gpu_helpers.py; the worst case measured is 8.6e-11).  That makes the restatement a
reference the device's 4 N terms can be compared with one by one (tests/test_gpu_decomposition.py).

The API surface: the library exports the two calls, null arguments are refused, the Python kernel fails the OpenMM way without
a device, the C++ mirror declares decompose()."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import openmm_agbnp_plugin_amd as P
from openmm_agbnp_plugin_amd import _lib
from tests.decomposition_restatement import TERMS, restate, surface_areas
from tests.edge_systems import NAMES, edge_systems
from tests.gpu_helpers import SAME

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("agbnp_hip_decompose_host", "agbnp_hip_decompose_device")


def check_identities(s, version, cutoff=None):
    energy, terms, o = restate(s.params(), s.pos, version=version, cutoff=cutoff)
    assert terms.shape == (4, s.n) and np.isfinite(terms).all()
    figures = dict(total=abs(terms.sum() - energy), cavity=abs(terms[0].sum() - (o.scalar("e_vol1") + o.scalar("e_vol2"))),
                   vdw=abs(terms[1].sum() - o.scalar("e_vdw")), gb=abs(terms[2].sum() + terms[3].sum() - o.scalar("e_gb")))
    print(s.name, version, cutoff, figures)
    for what, err in figures.items():
        assert err < SAME, f"{what}: {err:.3e}"
    assert (terms[0][s.ishydrogen != 0] == 0.0).all()
    if version == 0:
        assert (terms[1:] == 0.0).all()
    return terms


@pytest.mark.parametrize("version", [0, 1])
def test_the_planes_sum_to_the_oracle_energy_on_trpcage(version):
    s = P.load_system("trpcage")
    terms = check_identities(s, version)
    areas = surface_areas(terms, s.gamma)
    heavy = s.ishydrogen == 0
    assert areas[heavy].sum() > 1.0  # nm^2: a 20-residue protein
    assert (areas[~heavy] == 0.0).all()


def test_the_planes_sum_to_the_cutoff_oracle_energy_on_trpcage():
    s = P.load_system("trpcage")
    cut = check_identities(s, 1, cutoff=1.0)
    full = check_identities(s, 1)
    assert np.abs(cut[3] - full[3]).max() > 1e-3  # (the cutoff truncates pairs: another plane 3, other Born radii)
    energy_nocut, terms_nocut, _ = restate(s.params(), s.pos, cutoff=1.0, method=0)  # NoCutoff: the cutoff is inert
    np.testing.assert_array_equal(terms_nocut, full)


def test_the_planes_sum_to_the_oracle_energy_on_fixture264():
    check_identities(P.load_system("fixture264"), 1)


@pytest.mark.parametrize("name", NAMES)
def test_the_planes_sum_to_the_oracle_energy_on_the_edge_systems(name):
    check_identities(edge_systems()[name], 1)


def test_the_terms_are_named_in_the_header_order():
    assert P.DECOMPOSITION_TERMS == TERMS == ("cavity", "vdw", "gb_self", "gb_pair")
    assert _lib.DECOMPOSITION_TERMS == len(TERMS)
    header = open(os.path.join(ROOT, "include", "agbnp_hip.h")).read()
    assert "#define AGBNP_HIP_DECOMPOSITION_TERMS 4" in header


def test_the_decomposition_entry_points_are_exported():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "agbnp_hip.h")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS
        getattr(lib, name)
        assert f"int {name}(" in header


def test_a_null_context_is_an_invalid_argument():
    lib = _lib.load()
    e = C.c_double(0.0)
    pos, terms = np.zeros(3), np.zeros(4)
    dp = C.POINTER(C.c_double)
    assert lib.agbnp_hip_decompose_host(None, pos.ctypes.data_as(dp), terms.ctypes.data_as(dp), C.byref(e)) == _lib.ERR_INVALID_ARGUMENT
    assert lib.agbnp_hip_decompose_device(None, None, None, None, None) == _lib.ERR_INVALID_ARGUMENT


def test_decompose_without_a_device_fails_with_an_openmm_exception():
    """Without a device, initialize() and decompose() raise OpenMMException; with one, decompose() on a kernel that was never
    initialised does."""
    s = P.load_system("fixture264")
    if _lib.load().agbnp_hip_device_count() > 0:
        with pytest.raises(P.OpenMMException):
            P.HipCalcAGBNPForceKernel(device=0).decompose(s.pos)
        return
    k = P.HipCalcAGBNPForceKernel(device=0)
    with pytest.raises(P.OpenMMException):
        k.initialize(P.AGBNPForce.from_arrays(*s.params(), version=1))
    with pytest.raises(P.OpenMMException):
        k.decompose(s.pos)
    with pytest.raises(P.OpenMMException):
        k.decompose_device(0, 0)
    with pytest.raises(P.OpenMMException):
        P.AGBNPContext(P.AGBNPForce.from_arrays(*s.params(), version=1), device=0).getEnergyDecomposition()


def test_the_cpp_mirror_declares_decompose():
    subprocess.run(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-fsyntax-only", "-Wall", "-x", "c++", "-"],
                   input='#include "%s"\ndouble (AGBNPPlugin::HipCalcAGBNPForceKernel::*p)(const std::vector<double>&, std::vector<double>&) = '
                         '&AGBNPPlugin::HipCalcAGBNPForceKernel::decompose;\n' % os.path.join(ROOT, "cpp", "AGBNPForce.h"),
                   text=True, check=True)
