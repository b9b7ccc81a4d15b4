"""The OpenMM glue's energy-only path (openmm_glue/HipAGBNPKernels.cpp: execute with includeForces = false goes through
agbnp_hip_energy_openmm): tests/cxx/TestHipPlatformEnergyOnly.cpp, compiled against the OpenMM test double, calls
calcForcesAndEnergy(false, true) on a shuffled, padded "HIP" context and compares it with calcForcesAndEnergy(true, true)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOCK = os.path.join(ROOT, "tests", "openmm_mock")
GLUE = os.path.join(ROOT, "openmm_glue", "HipAGBNPKernels.cpp")
LIBDIR = os.path.join(ROOT, "openmm_agbnp_plugin_amd")
COMMON = ["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{MOCK}", f"-I{ROOT}/include", f"-I{ROOT}/openmm_glue",
          f"-I{MOCK}/agbnp_api"]


def build(tmp_path):
    exe = str(tmp_path / "TestHipPlatformEnergyOnly")
    subprocess.run(COMMON + ["-O1", os.path.join(ROOT, "tests", "cxx", "TestHipPlatformEnergyOnly.cpp"), GLUE,
                             os.path.join(LIBDIR, "libagbnp_hip.so"), "-L/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{LIBDIR}",
                             "-Wl,-rpath,/opt/rocm/lib", "-o", exe], check=True)
    return exe


def test_the_energy_only_program_builds(tmp_path):
    assert os.path.exists(build(tmp_path))


@pytest.mark.gpu
@pytest.mark.parametrize("version,precision", [(0, "double"), (1, "double"), (1, "mixed"), (1, "single")])
def test_calc_energy_without_forces_through_the_plugin(gpu_required, tmp_path, version, precision):
    exe = build(tmp_path)
    data = open(os.path.join(ROOT, "openmm_agbnp_plugin_amd", "data", "fixture264.dat")).read()
    out = subprocess.run([exe, str(version), precision], input=data, text=True, capture_output=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "PASS" in out.stdout
