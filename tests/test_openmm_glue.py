"""The OpenMM platform plugin of the engine (openmm_glue/HipAGBNPKernels.cpp): compiled against a test double of the
OpenMM API (tests/openmm_mock; OpenMM is not in the image) and -- on the GPU box -- run end to end: System + AGBNPForce ->
Context -> ForceImpl -> Platform("HIP").createKernel("CalcAGBNPForce") -> initialize -> execute, with the context's atoms
shuffled and padded, forces read back from the 2^32 fixed-point buffer, against the reference's printed known answers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOCK = os.path.join(ROOT, "tests", "openmm_mock")
GLUE = os.path.join(ROOT, "openmm_glue", "HipAGBNPKernels.cpp")
LIBDIR = os.path.join(ROOT, "openmm_agbnp_plugin_amd")
COMMON = ["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{MOCK}", f"-I{ROOT}/include", f"-I{ROOT}/openmm_glue"]


def build_test_program(tmp_path, name="TestHipPlatformAGBNPForce"):
    exe = str(tmp_path / name)
    subprocess.run(COMMON + ["-O1", f"-I{MOCK}/agbnp_api", os.path.join(ROOT, "tests", "cxx", name + ".cpp"), GLUE,
                             os.path.join(LIBDIR, "libagbnp_hip.so"), "-L/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{LIBDIR}",
                             "-Wl,-rpath,/opt/rocm/lib", "-o", exe], check=True)
    return exe


def test_glue_compiles_against_the_openmm_test_double():
    subprocess.run(COMMON + ["-fsyntax-only", "-Wall", f"-I{MOCK}/agbnp_api", GLUE], check=True)


def test_glue_exports_the_plugin_entry_points(tmp_path):
    """What OpenMM's plugin loader looks up in a platform plugin (ReferenceAGBNPKernelFactory.cpp:14-36)."""
    so = str(tmp_path / "libAGBNPPluginHip.so")
    subprocess.run(COMMON + ["-O1", "-shared", "-fPIC", f"-I{MOCK}/agbnp_api", GLUE, os.path.join(LIBDIR, "libagbnp_hip.so"),
                             "-L/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib", "-o", so], check=True)
    syms = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    for name in ("registerPlatforms", "registerKernelFactories", "registerAGBNPHipKernelFactories"):
        assert f" T {name}" in syms


def test_plugin_path_fails_cleanly_without_a_device(tmp_path):
    """No GPU: the test program must end with an OpenMM-style exception, not a crash (CPU-only check of the wiring)."""
    from openmm_agbnp_plugin_amd import _lib
    if _lib.load().agbnp_hip_device_count() > 0:
        pytest.skip("a HIP device is present")
    exe = build_test_program(tmp_path)
    data = open(os.path.join(ROOT, "openmm_agbnp_plugin_amd", "data", "fixture264.dat")).read()
    out = subprocess.run([exe, "1", "double"], input=data, text=True, capture_output=True, timeout=120)
    assert out.returncode == 2 and out.stdout.startswith("exception:")


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["double", "mixed", "single"])
@pytest.mark.parametrize("version", [0, 1])
def test_plugin_path_reproduces_the_reference_known_answers(gpu_required, tmp_path, version, precision):
    from tests.pins import REFERENCE_PRINTED
    exe = build_test_program(tmp_path)
    data = open(os.path.join(ROOT, "openmm_agbnp_plugin_amd", "data", "fixture264.dat")).read()
    out = subprocess.run([exe, str(version), precision], input=data, text=True, capture_output=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.split("\n")
    want = REFERENCE_PRINTED[version]
    if precision == "single":  # float positions and a float energy accumulator: 7 digits of a ~2500 kJ/mol energy
        assert abs(float(lines[0].split()[1]) - want["energy"]) < 0.05
    else:
        assert lines[0] == f"Energy: {want['energy']:g}"
        assert lines[1] == f"Energy: {want['energy_moved']:g}"
        assert f"Energy Change from Gradient: {want['change_from_gradient']:g}" in out.stdout
    assert "PASS" in out.stdout


@pytest.mark.gpu
def test_plugin_path_with_the_reference_blocking_check(gpu_required, tmp_path):
    """AGBNP_HIP_CHECK_MODE=finish: the reference's own protocol (stream synchronisation and a read of the overflow log after
    every evaluation) instead of the default wait for the device's verdict word; same numbers."""
    from tests.pins import REFERENCE_PRINTED
    exe = build_test_program(tmp_path)
    data = open(os.path.join(ROOT, "openmm_agbnp_plugin_amd", "data", "fixture264.dat")).read()
    env = dict(os.environ, AGBNP_HIP_CHECK_MODE="finish")
    out = subprocess.run([exe, "1", "double"], input=data, text=True, capture_output=True, timeout=300, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.split("\n")[0] == f"Energy: {REFERENCE_PRINTED[1]['energy']:g}"
    assert "PASS" in out.stdout


@pytest.mark.gpu
def test_plugin_path_in_poll_mode(gpu_required, tmp_path):
    """AGBNP_HIP_CHECK_MODE=poll: execute() looks at the engine's pinned status words instead of synchronising the stream
    every step; the numbers of a healthy run are the strict mode's."""
    from tests.pins import REFERENCE_PRINTED
    exe = build_test_program(tmp_path)
    data = open(os.path.join(ROOT, "openmm_agbnp_plugin_amd", "data", "fixture264.dat")).read()
    env = dict(os.environ, AGBNP_HIP_CHECK_MODE="poll")
    out = subprocess.run([exe, "1", "double"], input=data, text=True, capture_output=True, timeout=300, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.split("\n")[0] == f"Energy: {REFERENCE_PRINTED[1]['energy']:g}"
    assert "PASS" in out.stdout


PROTOCOL_STEPS = os.path.join(ROOT, "tests", "golden", "protocol_steps.dat")


def test_protocol_program_builds_and_fails_cleanly_without_a_device(tmp_path):
    """tests/cxx/TestHipPlatformProtocol.cpp compiles and links against the test double; without a GPU it ends with an
    OpenMM-style exception, not a crash."""
    from openmm_agbnp_plugin_amd import _lib
    exe = build_test_program(tmp_path, "TestHipPlatformProtocol")
    if _lib.load().agbnp_hip_device_count() > 0:
        return  # (the GPU tests below run it)
    data = open(os.path.join(ROOT, "openmm_agbnp_plugin_amd", "data", "fixture264.dat")).read()
    out = subprocess.run([exe, "double", PROTOCOL_STEPS], input=data, text=True, capture_output=True, timeout=120)
    assert out.returncode == 2 and out.stdout.startswith("exception:")


@pytest.mark.gpu
@pytest.mark.parametrize("check_mode", ["default", "finish"])
@pytest.mark.parametrize("precision", ["double", "mixed"])
def test_plugin_path_repeats_withheld_evaluations_to_the_oracle(gpu_required, systems, tmp_path, precision, check_mode):
    """The glue's repeat protocol MADE to repeat, against the oracle (not against six printed digits): the sequence of
    tests/golden/protocol_steps.dat through Context and calcForcesAndEnergy -- settle; a step that moves one heavy atom by 0.1 nm,
    which the engine withholds once (tests/test_gpu_openmm_entry.py::test_a_long_step_and_a_reorder_are_withheld_once_and_repeat_right
    shows that on this very step: nothing arrives in the buffers); a small step; HipContext::setAtomIndex with another order and a
    small step.  A glue that stops repeating hands back an evaluation without the AGBNP term.  Every evaluation's energy and forces
    are compared with the oracle at the positions the context held, at the tolerances of the execute_openmm tests; both blocking
    check modes (poll mode documents that a late-found withheld step is not repeated: not part of this)."""
    import numpy as np

    from oracle import Oracle
    from tests.gpu_helpers import TIGHT
    from tests.openmm_context import FIXED_POINT, protocol_geometries
    s = systems("fixture264")
    exe = build_test_program(tmp_path, "TestHipPlatformProtocol")
    data = open(os.path.join(ROOT, "openmm_agbnp_plugin_amd", "data", "fixture264.dat")).read()
    env = dict(os.environ)
    env.pop("AGBNP_HIP_CHECK_MODE", None)
    env.pop("AGBNP_HIP_CHECK_INTERVAL", None)
    if check_mode != "default":
        env["AGBNP_HIP_CHECK_MODE"] = check_mode
    out = subprocess.run([exe, precision, PROTOCOL_STEPS], input=data, text=True, capture_output=True, timeout=300, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    energies, pos, frc = [], [], []
    for line in out.stdout.split("\n"):
        w = line.split()
        if w[:1] == ["evaluation"]:
            assert int(w[1]) == len(energies) and w[2] == "energy"
            energies.append(float(w[3]))
            pos.append(np.full((s.n, 3), np.nan))
            frc.append(np.full((s.n, 3), np.nan))
        elif w[:1] in (["pos"], ["force"]):
            (pos if w[0] == "pos" else frc)[-1][int(w[1])] = [float(v) for v in w[2:5]]
    geoms, _ = protocol_geometries(s.pos)
    assert len(energies) == len(geoms) == 4
    oracle = Oracle(*s.params(), version=1)
    for k, geom in enumerate(geoms):
        assert np.abs(pos[k] - geom).max() < 1e-9  # the program took the steps of the shared file (mixed: float4 + correction of them)
        eo, fo = oracle.execute(pos[k])
        de, df = abs(energies[k] - eo), float(np.abs(frc[k] - fo).max())
        print(f"glue protocol ({precision}, {check_mode}), evaluation {k}: |dE|={de:.3e}  max|dF|={df:.3e}")
        assert df < FIXED_POINT
        assert de < TIGHT * max(1.0, abs(eo) * 1e-3)
