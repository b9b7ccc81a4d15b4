"""GPU box: set-pair interaction matrices (include/agbnp_hip.h: agbnp_hip_set_atom_sets, agbnp_hip_pair_matrix_host / _device;
DESIGN.md s.4r).  Every one of the S S cells against the NumPy restatement built from the CPU oracle's vectors
(tests/pair_matrix_restatement.py, pinned on the CPU by tests/test_pair_matrix_restatement.py) within TIGHT, and the matrix's sum
against the returned energy: with the residue fixtures, at the block edges crossed with the partitions where the new launch can
go wrong (one set, every atom its own, run length 1, sets across block edges, empty sets), in every mode, through the device
entry with its overflow log, and a context left exactly as a full evaluation leaves it.

The restatement of a geometry is computed once, as the matrix of every atom its own set, and shared (ATOMS): the matrix of a
partition is that one with the sets' one-hot matrix applied on both sides.  1dwc alone is restated with its partition directly."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import openmm_agbnp_plugin_amd as P
from openmm_agbnp_plugin_amd import _lib
from tests.edge_systems import edge_systems
from tests.gpu_helpers import SAME, TIGHT
from tests.gpu_helpers import energy_close as _energy_close
from tests.gpu_helpers import five  # noqa: F401
from tests.pair_matrix_restatement import restate_matrix

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ATOMS = {}


def residues(name):
    sets, labels = P.load_sets(os.path.join(GOLDEN, f"residues_{name}.txt"))
    return sets, len(labels)


def reference(s, tag, pos, sets, num_sets, version=1, cutoff=None, params=None):
    """(energy, M[num_sets, num_sets]) of the restatement at `pos`; the atoms' matrix once per (system, tag, version, cutoff)."""
    key = (s.name, tag, version, cutoff)
    if key not in ATOMS:
        e, atoms, _ = restate_matrix(params or s.params(), pos, np.arange(s.n), s.n, version=version, cutoff=cutoff)
        atoms.setflags(write=False)
        ATOMS[key] = (e, atoms)
    e, atoms = ATOMS[key]
    onehot = np.zeros((s.n, num_sets))
    onehot[np.arange(s.n), np.asarray(sets)] = 1.0
    return e, onehot.T @ atoms @ onehot


def _kernel(s, version=1, mode="reference", cutoff=None, sets=None, num_sets=None):
    k = P.HipCalcAGBNPForceKernel(device=0, mode=mode)
    force = P.AGBNPForce.from_arrays(*s.params(), version=version)
    if cutoff is not None:
        force.setNonbondedMethod(P.AGBNPForce.CutoffNonPeriodic)
        force.setCutoffDistance(cutoff)
    k.initialize(force)
    if sets is not None:
        k.set_atom_sets(sets, num_sets)
    return k


def cells_close(matrix, ref, tol=TIGHT):
    assert matrix.shape == ref.shape
    worst = float(np.abs(matrix - ref).max())
    print(f"worst |cell - restatement|: {worst:.3e} over {ref.shape[0]} x {ref.shape[1]} cells")
    assert worst < tol, f"cells differ by {worst:.3e}"


def check(k, pos, e_ref, ref):
    """One host call: every cell, the returned energy and the matrix's sum."""
    e, matrix = k.pair_matrix(pos)
    cells_close(matrix, ref)
    _energy_close(e, e_ref)
    _energy_close(float(matrix.sum()), e)
    assert int(k.scalar("last_evaluation_kind")) == 4
    return e, matrix


# ---- 1. the residue fixtures -------------------------------------------------------------------------------------------------
def test_trpcage_residues(gpu_required, systems, five):
    """20 residues, one of them not contiguous in atom order; another geometry on the same context; the Context stand-in."""
    s = systems("trpcage")
    sets, S = residues("trpcage")
    k = _kernel(s, sets=sets)
    assert k.num_atom_sets() == S == 20
    e, m = check(k, s.pos, *reference(s, "file", s.pos, sets, S))
    assert np.abs(m - m.T).max() < SAME
    f = np.zeros((s.n, 3))
    _energy_close(e, k.execute(s.pos, f))
    assert int(k.scalar("last_evaluation_kind")) == 0
    check(k, s.jittered(1), *reference(s, "jitter1", s.jittered(1), sets, S))
    ctx = P.AGBNPContext(P.AGBNPForce.from_arrays(*s.params(), version=1), device=0)
    ctx.setPositions(s.pos)
    e2, m2 = ctx.getInteractionMatrix(sets)
    cells_close(m2, reference(s, "file", s.pos, sets, S)[1])
    assert abs(e2 - e) < SAME
    e3, m3 = ctx.getInteractionMatrix(sets, groups=2)
    assert e3 == 0.0 and m3.shape == (S, S) and not m3.any()


def test_1dwc_residues(gpu_required, systems, five):
    """Many tiles (2145), 258 sets, about nine of them to a block."""
    s = systems("1dwc")
    sets, S = residues("1dwc")
    k = _kernel(s, sets=sets)
    e_ref, ref, _ = restate_matrix(s.params(), s.pos, sets, S)
    check(k, s.pos, e_ref, ref)


# ---- 2. block edges x partitions ---------------------------------------------------------------------------------------------
EDGES = ("size_0_1", "size_1_33", "size_65_65", "size_129_257", "size_257_513", "born_clamp_strip_27")
PARTITIONS = {
    "one_set": lambda n: (np.zeros(n, dtype=int), 1),
    "every_atom": lambda n: (np.arange(n), n),                       # the full accumulator, run length 1
    "modulo_3": lambda n: (np.arange(n) % 3, 3),                     # non-contiguous, run length 1, nine cells
    "straddling": lambda n: ((np.arange(n) + 8) // 16, (n + 7) // 16 + 1),  # sets across every block edge
    "empty_sets": lambda n: (2 * (np.arange(n) // 16), 2 * ((n + 15) // 16)),  # the odd sets are empty
}


@pytest.mark.parametrize("partition", list(PARTITIONS))
@pytest.mark.parametrize("name", EDGES)
def test_block_edges_and_partitions(gpu_required, five, name, partition):
    s = edge_systems()[name]
    sets, S = PARTITIONS[partition](s.n)
    k = _kernel(s, sets=sets, num_sets=S)
    assert k.num_atom_sets() == S
    e, m = check(k, s.pos, *reference(s, "file", s.pos, sets, S))
    if partition == "one_set":
        _energy_close(m[0, 0], e)
    if partition == "empty_sets":
        assert (m[1::2] == 0.0).all() and (m[:, 1::2] == 0.0).all()


# ---- 3. versions and modes ---------------------------------------------------------------------------------------------------
def test_version_0_fills_the_diagonal_only(gpu_required, systems, five):
    s = systems("fixture264")
    sets, S = PARTITIONS["straddling"](s.n)
    k = _kernel(s, version=0, sets=sets, num_sets=S)
    e, m = check(k, s.pos, *reference(s, "file", s.pos, sets, S, version=0))
    assert (m - np.diag(np.diag(m)) == 0.0).all()
    _energy_close(float(np.trace(m)), e)
    assert abs(e - 872.5144) < 1e-3


def test_fast_mode_with_a_cutoff(gpu_required, systems, five):
    s = systems("trpcage")
    sets, S = residues("trpcage")
    k = _kernel(s, mode="fast", cutoff=1.0, sets=sets)
    check(k, s.pos, *reference(s, "file", s.pos, sets, S, cutoff=1.0))


def test_fast_mode_without_a_cutoff_is_the_reference_mode(gpu_required, systems, five):
    s = systems("trpcage")
    sets, S = residues("trpcage")
    e_fast, m_fast = _kernel(s, mode="fast", sets=sets).pair_matrix(s.pos)
    e_ref, m_ref = _kernel(s, sets=sets).pair_matrix(s.pos)
    assert np.abs(m_fast - m_ref).max() < SAME and abs(e_fast - e_ref) < SAME
    cells_close(m_fast, reference(s, "file", s.pos, sets, S)[1])


def test_fast_single_cells_are_those_of_the_fp64_fast_mode(gpu_required, systems, five):
    s = systems("trpcage")
    sets, S = residues("trpcage")
    k = _kernel(s, mode="fast+single", cutoff=1.0, sets=sets)
    before = k.energy(s.pos)
    check(k, s.pos, *reference(s, "file", s.pos, sets, S, cutoff=1.0))
    assert abs(k.energy(s.pos) - before) < 1e-6  # (the context stays in its mode)


def test_deterministic_mode_is_bit_identical(gpu_required, systems, five):
    """A cell receives at most 24 x 24 rounded contributions of at most 2^-37 each: under 5e-9, inside TIGHT."""
    s = systems("trpcage")
    sets, S = residues("trpcage")
    k = _kernel(s, mode="deterministic", sets=sets)
    e1, m1 = check(k, s.pos, *reference(s, "file", s.pos, sets, S))
    e2, m2 = k.pair_matrix(s.pos)
    assert e1 == e2 and np.array_equal(m1, m2)


# ---- 4. device entry ---------------------------------------------------------------------------------------------------------
def test_the_device_entry_adds(gpu_required, systems, five):
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    sets, S = residues("trpcage")
    k = _kernel(s, sets=sets)
    k.execute(s.pos, np.zeros((s.n, 3)))
    e_ref, ref = reference(s, "jitter1", s.jittered(1), sets, S)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    pos = torch.tensor(s.jittered(1), dtype=torch.float64, device=dev).contiguous()
    pos0 = pos.clone()
    matrix = torch.full((S, S), 1.0, dtype=torch.float64, device=dev)
    ene = torch.full((1,), 2.0, dtype=torch.float64, device=dev)
    lone = torch.zeros((S, S), dtype=torch.float64, device=dev)
    k.pair_matrix_device(pos.data_ptr(), matrix.data_ptr(), ene.data_ptr(), stream)
    k.pair_matrix_device(pos.data_ptr(), matrix.data_ptr(), ene.data_ptr(), stream)
    k.pair_matrix_device(pos.data_ptr(), lone.data_ptr(), None, stream)  # d_energy = NULL is accepted
    assert int(k.scalar("last_evaluation_kind")) == 4
    assert k.finish(stream) == 0, (k.withheld(), int(k.scalar("overflow_kinds")))
    torch.cuda.synchronize()
    cells_close(matrix.cpu().numpy(), 1.0 + 2.0 * ref, 2 * TIGHT)
    _energy_close(ene.item(), 2.0 + 2.0 * e_ref, 2 * TIGHT)
    cells_close(lone.cpu().numpy(), ref)
    assert torch.equal(pos, pos0)


def test_a_jump_is_withheld_and_a_hint_prevents_it(gpu_required, systems, five):
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    sets, S = residues("trpcage")
    k = _kernel(s, sets=sets)
    k.execute(s.pos, np.zeros((s.n, 3)))
    assert int(k.scalar("launches")) == 5
    heavy = np.flatnonzero(s.ishydrogen == 0)
    moved = s.pos.copy()
    moved[heavy[len(heavy) // 2], 0] += 0.06
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    pos = torch.tensor(moved, dtype=torch.float64, device=dev).contiguous()
    matrix = torch.full((S, S), 1.0, dtype=torch.float64, device=dev)
    ene = torch.full((1,), 2.0, dtype=torch.float64, device=dev)
    k.pair_matrix_device(pos.data_ptr(), matrix.data_ptr(), ene.data_ptr(), stream)
    assert k.finish(stream) == 1 and list(k.withheld()) == [0]
    torch.cuda.synchronize()
    assert (matrix == 1.0).all().item() and ene.item() == 2.0  # nothing was added to either output
    # the same call after the hint is complete (the masks of the withheld evaluation lie at `moved`: jump back first)
    k.execute(s.pos, np.zeros((s.n, 3)))
    k.expect_jump()
    k.pair_matrix_device(pos.data_ptr(), matrix.data_ptr(), ene.data_ptr(), stream)
    assert k.finish(stream) == 0, (k.withheld(), int(k.scalar("overflow_kinds")))
    e_ref, ref = reference(s, "moved", moved, sets, S)
    cells_close(matrix.cpu().numpy(), 1.0 + ref)
    _energy_close(ene.item(), 2.0 + e_ref)
    assert int(k.scalar("launches")) == 5
    # the host entry point across a jump repeats by itself
    check(k, s.pos, *reference(s, "file", s.pos, sets, S))


# ---- 5. the partition's life -------------------------------------------------------------------------------------------------
def test_a_replaced_partition_and_a_refused_one(gpu_required, systems, five):
    s = systems("trpcage")
    sets, S = residues("trpcage")
    k = _kernel(s, sets=sets)
    check(k, s.pos, *reference(s, "file", s.pos, sets, S))
    state = (k.generation(), int(k.scalar("launches")), int(k.scalar("energy_only_launches")))
    mod3 = np.arange(s.n) % 3
    k.set_atom_sets(mod3)
    assert k.num_atom_sets() == 3
    assert (k.generation(), int(k.scalar("launches")), int(k.scalar("energy_only_launches"))) == state
    check(k, s.pos, *reference(s, "file", s.pos, mod3, 3))  # (no stale tables)
    # refused by the library itself: the partition before stays in force
    lib = _lib.load()
    bad = np.ascontiguousarray(mod3, dtype=np.int32)
    bad[5] = 3
    ip = bad.ctypes.data_as(C.POINTER(C.c_int))
    assert lib.agbnp_hip_set_atom_sets(k._h, s.n, ip, 3) == _lib.ERR_INVALID_ARGUMENT
    assert "set" in _lib.last_error(k._h)
    assert lib.agbnp_hip_set_atom_sets(k._h, s.n - 1, ip, 4) == _lib.ERR_INVALID_ARGUMENT
    assert lib.agbnp_hip_set_atom_sets(k._h, s.n, None, 4) == _lib.ERR_INVALID_ARGUMENT
    assert lib.agbnp_hip_set_atom_sets(k._h, s.n, ip, 0) == _lib.ERR_INVALID_ARGUMENT
    assert lib.agbnp_hip_set_atom_sets(k._h, s.n, ip, 2049) == _lib.ERR_INVALID_ARGUMENT
    assert lib.agbnp_hip_pair_matrix_host(k._h, None, None, None) == _lib.ERR_INVALID_ARGUMENT
    assert lib.agbnp_hip_pair_matrix_device(k._h, None, None, None, None) == _lib.ERR_INVALID_ARGUMENT
    with pytest.raises(P.OpenMMException):
        k.set_atom_sets(bad, 3)
    assert k.num_atom_sets() == 3
    check(k, s.pos, *reference(s, "file", s.pos, mod3, 3))


def test_update_parameters_keeps_the_partition(gpu_required, systems, five):
    s = systems("trpcage")
    sets, S = residues("trpcage")
    force = P.AGBNPForce.from_arrays(*s.params(), version=1)
    k = P.HipCalcAGBNPForceKernel(device=0)
    k.initialize(force)
    k.set_atom_sets(sets)
    e0, m0 = k.pair_matrix(s.pos)
    for i in range(s.n):
        r, g, a, q, h = force.getParticleParameters(i)
        force.setParticleParameters(i, r, g, a, 0.5 * q, h)
    k.copyParametersToContext(force)
    assert k.num_atom_sets() == S
    halved = (s.radius, s.gamma, s.alpha, 0.5 * s.charge, s.ishydrogen)
    e1, m1 = check(k, s.pos, *reference(s, "halved", s.pos, sets, S, params=halved))
    off = ~np.eye(S, dtype=bool)
    assert np.abs(m1[off] - 0.25 * m0[off]).max() < TIGHT  # (the Born radii do not depend on the charges)


def test_the_context_is_left_as_a_full_evaluation_leaves_it(gpu_required, systems, five):
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    sets, S = residues("trpcage")
    k, twin = _kernel(s, sets=sets), _kernel(s)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    geoms = torch.tensor(np.stack([s.jittered(1), s.jittered(2)]), dtype=torch.float64, device=dev).contiguous()
    out = {}
    for who, kernel in (("with", k), ("without", twin)):
        kernel.execute(s.pos, np.zeros((s.n, 3)))
        state = (kernel.generation(), int(kernel.scalar("launches")), int(kernel.scalar("energy_only_launches")))
        assert state[1:] == (5, 4)
        frc = torch.zeros((s.n, 3), dtype=torch.float64, device=dev)
        ene = torch.zeros((1,), dtype=torch.float64, device=dev)
        if who == "with":
            matrix = torch.zeros((S, S), dtype=torch.float64, device=dev)
            kernel.pair_matrix_device(geoms[0].data_ptr(), matrix.data_ptr(), None, stream)
            assert int(kernel.scalar("last_evaluation_kind")) == 4
        else:
            spare = torch.zeros((1,), dtype=torch.float64, device=dev)
            kernel.energy_device(geoms[0].data_ptr(), spare.data_ptr(), stream)
        kernel.execute_device(geoms[1].data_ptr(), frc.data_ptr(), ene.data_ptr(), stream)
        assert int(kernel.scalar("last_evaluation_kind")) == 0
        assert kernel.finish(stream) == 0
        assert (kernel.generation(), int(kernel.scalar("launches")), int(kernel.scalar("energy_only_launches"))) == state
        out[who] = (ene.item(), frc.cpu().numpy())
    assert abs(out["with"][0] - out["without"][0]) < SAME and np.abs(out["with"][1] - out["without"][1]).max() < SAME
    cells_close(matrix.cpu().numpy(), reference(s, "jitter1", s.jittered(1), sets, S)[1])


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------
def test_pair_matrix_device_refuses_a_stream_capture(gpu_required, systems, five):
    """Inside a capture the call fails with INVALID_ARGUMENT, launches nothing, and the capture ends cleanly and replays."""
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    sets, S = residues("trpcage")
    k = _kernel(s, sets=sets)
    k.execute(s.pos, np.zeros((s.n, 3)))
    dev = torch.device("cuda:0")
    pos = torch.tensor(s.jittered(1), dtype=torch.float64, device=dev).contiguous()
    matrix = torch.zeros((S, S), dtype=torch.float64, device=dev)
    ene = torch.zeros((1,), dtype=torch.float64, device=dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ene.fill_(1.0)
        with pytest.raises(P.OpenMMException, match="captur"):
            k.pair_matrix_device(pos.data_ptr(), matrix.data_ptr(), ene.data_ptr(), torch.cuda.current_stream().cuda_stream)
    ene.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert ene.item() == 1.0 and not matrix.any().item()
    assert int(k.scalar("launches")) == 5 and int(k.scalar("energy_only_launches")) == 4
    check(k, s.jittered(1), *reference(s, "jitter1", s.jittered(1), sets, S))


def test_without_a_partition_the_calls_are_refused(gpu_required, systems, five):
    s = systems("trpcage")
    k = _kernel(s)
    assert k.num_atom_sets() == 0
    with pytest.raises(P.OpenMMException, match="no partition has been set"):
        k.pair_matrix(s.pos)
    with pytest.raises(P.OpenMMException, match="no partition has been set"):
        k.pair_matrix_device(1, 2)
    f = np.zeros((s.n, 3))
    k.execute(s.pos, f)  # (the context goes on)
    assert f.any()


# ---- 7. the C++ mirror -------------------------------------------------------------------------------------------------------
def test_cxx_mirror(gpu_required, systems, five, tmp_path):
    """tests/cxx/TestHipPairMatrix.cpp through cpp/AGBNPForce.h."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(root, "openmm_agbnp_plugin_amd")
    exe = str(tmp_path / "TestHipPairMatrix")
    subprocess.run(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    os.path.join(root, "tests", "cxx", "TestHipPairMatrix.cpp"), "-o", exe, os.path.join(libdir, "libagbnp_hip.so"),
                    "-L/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    x = systems("trpcage")
    sets, _ = residues("trpcage")
    path = tmp_path / "trpcage.txt"
    r, g, a, q, h = x.params()
    np.savetxt(path, np.column_stack([r, g, a, q, np.asarray(h, dtype=float), x.pos, sets.astype(float)]), fmt="%.17g")
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
