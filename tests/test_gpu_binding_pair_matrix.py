"""GPU box: the set-pair matrix of a binding energy (include/agbnp_hip.h: agbnp_hip_binding_set_atom_sets,
agbnp_hip_binding_pair_matrix_device / _host) -- D[a][b] = M_RL[a][b] - M_R[a][b] - M_L[a][b] from ONE pair-matrix
group over the complex, its receptor and its ligand, each with the partition restricted to its atoms, gated on all three verdicts
on the device.  The reference is tests/binding_pair_matrix_restatement.py (pinned on the CPU by
tests/test_binding_pair_matrix_restatement.py); the restatement of a case at a geometry is computed once and shared (REFS).

Tolerances: every one of the S S cells within 3 TIGHT (a difference of three member cells, TIGHT = 1e-7 each), u within 3 TIGHT
on energy_close's scale (max(1, 1e-3 |E|)), as tests/test_gpu_binding_decomposition.py has it; row sums against the per-set sums of
BindingEnergy.decompose within 5 TIGHT (two member terms there, three member cells here); symmetry within SAME = 1e-9."""
import ctypes as C
import os

import numpy as np
import pytest

import openmm_agbnp_plugin_amd as P
from openmm_agbnp_plugin_amd import _lib
from tests.binding_pair_matrix_restatement import restate
from tests.binding_restatement import restate as restate_binding
from tests.edge_systems import edge_systems
from tests.gpu_helpers import SAME, TIGHT
from tests.gpu_helpers import five_groups  # noqa: F401

pytestmark = pytest.mark.gpu
SENTINEL = -1234.5678
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REFS = {}
WORST = [0.0]  # the worst |cell - restatement| this file has seen (printed by every comparison)


def residues(name):
    sets, labels = P.load_sets(os.path.join(GOLDEN, f"residues_{name}.txt"))
    return np.asarray(sets), len(labels)


def straddling(n):
    return (np.arange(n) + 8) // 16, (n + 7) // 16 + 1


def reference(s, ligand, sets, S, tag, pos, version=1, cutoff=None, params=None):
    """(D[S, S], u, scale) of the restatement at `pos`, once per case and geometry tag."""
    key = (s.name, tuple(sorted(int(a) for a in ligand)), tuple(int(a) for a in sets), version, cutoff, tag)
    if key not in REFS:
        p = params or s.params()
        d, u = restate(p, ligand, pos, sets, S, version=version, cutoff=cutoff)
        energies = restate_binding(p, ligand, pos, 0.35, version=version, cutoff=cutoff)[3]
        d.setflags(write=False)
        REFS[key] = (d, u, max(1.0, 1e-3 * max(abs(x) for x in energies)))
    return REFS[key]


def _binding(s, ligand, sets=None, S=None, version=1, mode="reference", cutoff=None):
    force = P.AGBNPForce.from_arrays(*s.params(), version=version)
    if cutoff is not None:
        force.setNonbondedMethod(P.AGBNPForce.CutoffNonPeriodic)
        force.setCutoffDistance(cutoff)
    b = P.BindingEnergy(force, ligand, device=0, mode=mode)
    if sets is not None:
        b.set_atom_sets(sets, S)
    return b


def check(got, ref, count=1, fill=(0.0, 0.0), what=""):
    """got = (D[S, S], u) as the engine gave them -- `count` evaluations of this reference added to `fill`."""
    d_ref, u_ref, unit = ref
    d, u = got
    d = np.asarray(d)
    assert d.shape == d_ref.shape
    worst = float(np.abs(d - fill[0] - count * d_ref).max())
    du = abs(u - fill[1] - count * u_ref)
    WORST[0] = max(WORST[0], worst / count)
    print(f"binding matrix {what}: worst |cell - restatement| {worst:.3e} over {d.shape[0]} x {d.shape[1]} cells  |du| {du:.2e}  "
          f"(scale {unit:.3f}; file so far {WORST[0]:.3e})")
    assert worst < count * 3.0 * TIGHT, f"cells differ by {worst:.3e}"
    assert du < count * 3.0 * TIGHT * unit, f"u differs by {du:.3e}"


class Buffers:
    """The caller's device buffers: positions, the matrix [S, S] and u (torch tensors), pre-filled."""

    def __init__(self, torch, n, S, fill=(0.0, 0.0)):
        dev = torch.device("cuda:0")
        self.torch, self.fill = torch, fill
        self.pos = torch.zeros((n, 3), dtype=torch.float64, device=dev)
        self.matrix = torch.full((S, S), fill[0], dtype=torch.float64, device=dev)
        self.u = torch.full((1,), fill[1], dtype=torch.float64, device=dev)
        self.stream = torch.cuda.current_stream().cuda_stream

    def load(self, geom):
        self.pos.copy_(self.torch.tensor(np.asarray(geom), dtype=self.torch.float64))

    def evaluate(self, b, with_u=True):
        b.pair_matrix_device(self.pos.data_ptr(), self.matrix.data_ptr(), self.u.data_ptr() if with_u else None, self.stream)

    def result(self):
        return self.matrix.cpu().numpy(), self.u.item()

    def snapshot(self):
        return self.matrix.clone(), self.u.clone()

    def unchanged_since(self, snap):
        return all(self.torch.equal(a, b) for a, b in zip((self.matrix, self.u), snap))


def _member_kinds(b):
    return [int(b.member(m).scalar("last_evaluation_kind")) for m in range(3)]


# ---- 1. parity with the restatement, index maps and block edges --------------------------------------------------------------
CASES = {  # name -> (system, ligand atoms, version, partition)
    "trpcage_0_15_residues": ("trpcage", range(0, 16), 1, "residues"),
    "trpcage_every_third_mod3": ("trpcage", range(0, 272, 3), 1, "mod3"),
    "fixture264_200_263_v0_straddling": ("fixture264", range(200, 264), 0, "straddling"),
    "fixture264_200_263_v1_straddling": ("fixture264", range(200, 264), 1, "straddling"),
    "size_257_513_last_257_atoms": ("size_257_513", range(256, 513), 1, "atoms"),
    "size_257_513_atom_256_atoms": ("size_257_513", [256], 1, "atoms"),
}


def _case(systems, case):
    name, ligand, version, partition = CASES[case]
    s = edge_systems()[name] if name.startswith("size_") else systems(name)
    if partition == "residues":
        sets, S = residues(name)
    elif partition == "mod3":
        sets, S = np.arange(s.n) % 3, 3
    elif partition == "straddling":
        sets, S = straddling(s.n)
    else:
        sets, S = np.arange(s.n), s.n
    return s, list(ligand), version, sets, S


@pytest.mark.parametrize("case", sorted(CASES))
def test_parity_with_the_restatement(gpu_required, systems, five_groups, case):
    """A contiguous ligand that cuts residues (mixed sets); a ligand strewn over the complex whose set IS one of three; both
    versions with sets across every block edge; every atom its own set (513 sets: empty sets in both sub-systems, the full
    accumulator) with a ligand that is the second half, and with one atom.  The host form and the device form; D.sum() and u are
    the u of energy_device; the rows are the sets' shares of decompose(); D is symmetric."""
    torch = pytest.importorskip("torch")
    s, ligand, version, sets, S = _case(systems, case)
    b = _binding(s, ligand, sets, S, version=version)
    assert b.num_atom_sets() == S and [b.member(m).num_atom_sets() for m in range(3)] == [S, S, S]
    ref = reference(s, ligand, sets, S, "file", s.pos, version=version)
    d, u = b.pair_matrix(s.pos)
    check((d, u), ref, what=case + " host")
    assert _member_kinds(b) == [4, 4, 4]
    assert np.abs(d - d.T).max() < SAME
    if version == 0:
        assert (d - np.diag(np.diag(d)) == 0.0).all()
    terms, u_terms = b.decompose(s.pos)
    shares = np.zeros(S)
    np.add.at(shares, sets, terms.sum(axis=0))
    worst_row = np.abs(d.sum(axis=1) - shares).max()
    print(f"{case}: worst |row sum - share of decompose()| {worst_row:.3e}")
    assert worst_row < 5.0 * TIGHT
    buf = Buffers(torch, s.n, S)
    buf.load(s.pos)
    buf.evaluate(b)
    e_word = torch.zeros((2,), dtype=torch.float64, device=buf.pos.device)
    b.energy_device(buf.pos.data_ptr(), 0.35, e_word[0:1].data_ptr(), e_word[1:2].data_ptr(), buf.stream)
    assert b.finish(buf.stream) == 0 and b.withheld() == []
    got = buf.result()
    check(got, ref, what=case + " device")
    assert np.abs(got[0] - got[0].T).max() < SAME
    u_energy = e_word[1].item()
    print(f"{case}: sum D {got[0].sum()!r}  u (pair_matrix) {got[1]!r}  u (energy_device) {u_energy!r}")
    assert abs(got[0].sum() - u_energy) < 3.0 * TIGHT * ref[2]
    assert abs(got[1] - u_energy) < SAME * ref[2] and abs(u - u_energy) < SAME * ref[2] and abs(u_terms - u_energy) < SAME * ref[2]


def test_one_launch_set_and_the_order_of_the_ligand_list(gpu_required, systems, five_groups):
    s = systems("trpcage")
    sets, S = residues("trpcage")
    down = _binding(s, list(range(15, -1, -1)), sets)
    up = _binding(s, list(range(16)), sets)
    got_down, got_up = down.pair_matrix(s.pos), up.pair_matrix(s.pos)
    check(got_down, reference(s, range(16), sets, S, "file", s.pos), what="descending list")
    assert np.abs(got_down[0] - got_up[0]).max() < SAME and abs(got_down[1] - got_up[1]) < SAME
    assert _member_kinds(down) == [4, 4, 4]
    assert [int(down.member(m).scalar("group_members")) for m in range(3)] == [3, 3, 3]  # one launch set: 1 + 5 + 1 launches
    assert [int(down.member(m).scalar("energy_only_launches")) + 1 for m in range(3)] == [5, 5, 5]


# ---- 2. the device entry adds; NULL d_binding_energy --------------------------------------------------------------------------
def test_the_device_entry_adds_and_takes_no_u(gpu_required, systems, five_groups):
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    sets, S = residues("trpcage")
    ligand = list(range(16))
    b = _binding(s, ligand, sets)
    ref = reference(s, ligand, sets, S, "jitter1", s.jittered(1))
    buf = Buffers(torch, s.n, S, fill=(1.0, 2.0))
    buf.load(s.jittered(1))
    pos0 = buf.pos.clone()
    buf.evaluate(b)
    buf.evaluate(b)
    buf.evaluate(b, with_u=False)
    assert b.finish(buf.stream) == 0
    d, u = buf.result()
    check((d, 2.0 + 3.0 * ref[1]), ref, count=3, fill=(1.0, 2.0), what="three calls, cells")
    check((1.0 + 2.0 * ref[0], u), ref, count=2, fill=(1.0, 2.0), what="two calls with u")
    assert torch.equal(buf.pos, pos0)


# ---- 3. withheld: all or nothing, and the staging is cleared ------------------------------------------------------------------
def test_a_jump_of_a_ligand_atom_withholds_everything(gpu_required, systems, five_groups):
    """One heavy atom of the ligand jumps 0.1 nm: the ligand and the complex are withheld, the receptor is complete -- nothing
    reaches the caller's sentinel-filled buffers, bit for bit, and finish() reports one.  The next call on the same buffers is
    right: the receptor's matrix and energy did not stay in the staging words."""
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    sets, S = residues("trpcage")
    ligand = list(range(16))
    b = _binding(s, ligand, sets)
    buf = Buffers(torch, s.n, S, fill=(SENTINEL, SENTINEL))
    buf.load(s.pos)
    buf.evaluate(b)
    assert b.finish(buf.stream) == 0
    check(buf.result(), reference(s, ligand, sets, S, "file", s.pos), fill=(SENTINEL, SENTINEL), what="before the jump")
    heavy = np.flatnonzero(s.ishydrogen == 0)
    atom = int(heavy[heavy < 16][2])
    moved = s.pos.copy()
    moved[atom, 0] += 0.1
    buf.matrix.fill_(SENTINEL)
    buf.u.fill_(SENTINEL)
    buf.load(moved)
    snap = buf.snapshot()
    buf.evaluate(b)
    assert b.finish(buf.stream) == 1 and b.withheld() == [0]
    assert buf.unchanged_since(snap), "a withheld binding matrix reached the caller's buffers"
    buf.evaluate(b)  # the same call on the same buffers: complete now (the masks lie at the moved positions)
    assert b.finish(buf.stream) == 0
    ref = reference(s, ligand, sets, S, f"moved{atom}", moved)
    check(buf.result(), ref, fill=(SENTINEL, SENTINEL), what="the next call after the ligand's jump")
    b.expect_jump()
    back = Buffers(torch, s.n, S)
    back.load(s.pos)
    back.evaluate(b)
    assert b.finish(back.stream) == 0
    check(back.result(), reference(s, ligand, sets, S, "file", s.pos), what="hinted jump back")


# ---- 4. interleaving -----------------------------------------------------------------------------------------------------------
def test_interleaved_with_the_other_binding_calls(gpu_required, systems, five_groups):
    torch = pytest.importorskip("torch")
    from tests.test_gpu_binding import Buffers as ForceBuffers
    from tests.test_gpu_binding import check as check_forces
    from tests.test_gpu_binding import reference as force_reference
    from tests.test_gpu_binding_decomposition import Buffers as PlaneBuffers
    from tests.test_gpu_binding_decomposition import check as check_planes
    from tests.test_gpu_binding_decomposition import reference as plane_reference
    s = systems("trpcage")
    sets, S = residues("trpcage")
    ligand = list(range(16))
    b = _binding(s, ligand, sets)
    geoms = [s.jittered(k) for k in range(1, 7)]
    full = [ForceBuffers(torch, s.n) for _ in range(2)]
    dec = [PlaneBuffers(torch, s.n) for _ in range(2)]
    mat = [Buffers(torch, s.n, S) for _ in range(2)]
    order = [(mat[0], "M"), (full[0], "F"), (dec[0], "D"), (mat[1], "M"), (dec[1], "D"), (full[1], "F")]
    for (x, what), g in zip(order, geoms):
        x.load(g)
    torch.cuda.synchronize()
    for x, what in order:
        if what == "F":
            x.execute(b, 0.35)
        elif what == "D":
            x.decompose(b)
        else:
            x.evaluate(b)
        assert _member_kinds(b) == [dict(F=0, D=3, M=4)[what]] * 3
    assert b.finish(mat[0].stream) == 0 and b.withheld() == []
    for k, ((x, what), g) in enumerate(zip(order, geoms), start=1):
        if what == "M":
            check(x.result(), reference(s, ligand, sets, S, f"jitter{k}", g), what=f"call {k}")
        elif what == "D":
            check_planes(x.result(), plane_reference(s, ligand, f"jitter{k}", g), what=f"call {k}")
        else:
            check_forces(x.result(), force_reference(s, ligand, f"jitter{k}", g), 0.35, what=f"call {k}")


# ---- 5. modes ------------------------------------------------------------------------------------------------------------------
def test_deterministic_mode_is_bit_identical(gpu_required, systems, five_groups):
    """A member's cell receives at most 24 x 24 rounded contributions of at most 2^-37 each, under 5e-9; D is a
    difference of three such cells: under 1.5e-8, inside 3 TIGHT.  The combine is elementwise: two calls give the same bits."""
    s = systems("trpcage")
    sets, S = residues("trpcage")
    ligand = list(range(16))
    b = _binding(s, ligand, sets, mode="deterministic")
    d1, u1 = b.pair_matrix(s.pos)
    d2, u2 = b.pair_matrix(s.pos)
    check((d1, u1), reference(s, ligand, sets, S, "file", s.pos), what="deterministic")
    assert np.array_equal(d1, d2) and u1 == u2
    assert [int(b.member(m).scalar("group_members")) for m in range(3)] == [0, 0, 0]  # (every member ran alone)


# ---- 6. the partition's life -----------------------------------------------------------------------------------------------------
def test_a_replaced_partition_with_another_size_and_a_refused_one(gpu_required, systems, five_groups):
    """20 sets, then 3, then 20 again through the device form: the staging buffer is remade for every S and no cell of the old
    one is left.  A partition the library refuses leaves the old one in force in all three members."""
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    sets, S = residues("trpcage")
    mod3 = np.arange(s.n) % 3
    ligand = list(range(16))
    b = _binding(s, ligand, sets)
    for part, n in ((sets, S), (mod3, 3), (sets, S)):
        b.set_atom_sets(part)
        assert b.num_atom_sets() == n and [b.member(m).num_atom_sets() for m in range(3)] == [n] * 3
        buf = Buffers(torch, s.n, n)
        buf.load(s.pos)
        buf.evaluate(b)
        assert b.finish(buf.stream) == 0
        check(buf.result(), reference(s, ligand, part, n, "file", s.pos), what=f"{n} sets")
    lib = _lib.load()
    bad = np.ascontiguousarray(mod3, dtype=np.int32)
    bad[s.n - 1] = 3  # (a receptor atom: the complex's own check would pass the ligand's restriction)
    ip = bad.ctypes.data_as(C.POINTER(C.c_int))
    assert lib.agbnp_hip_binding_set_atom_sets(b._h, s.n, ip, 3) == _lib.ERR_INVALID_ARGUMENT
    assert "set" in _lib.last_error(None)
    assert lib.agbnp_hip_binding_set_atom_sets(b._h, s.n - 1, ip, 4) == _lib.ERR_INVALID_ARGUMENT
    assert lib.agbnp_hip_binding_set_atom_sets(b._h, s.n, None, 4) == _lib.ERR_INVALID_ARGUMENT
    assert lib.agbnp_hip_binding_set_atom_sets(b._h, s.n, ip, 0) == _lib.ERR_INVALID_ARGUMENT
    assert lib.agbnp_hip_binding_set_atom_sets(b._h, s.n, ip, 2049) == _lib.ERR_INVALID_ARGUMENT
    with pytest.raises(P.OpenMMException):
        b.set_atom_sets(bad, 3)
    assert b.num_atom_sets() == S and [b.member(m).num_atom_sets() for m in range(3)] == [S] * 3
    check(b.pair_matrix(s.pos), reference(s, ligand, sets, S, "file", s.pos), what="after the refusals")


def test_the_host_forms_across_partitions_of_another_size(gpu_required, systems, five_groups):
    """One binding through the HOST forms alone: the matrix with 20 sets, the planes, the matrix with 3 sets, the planes, the
    matrix with 20 again.  The matrix's host staging is remade for every S (its positions, its S S cells and u lie elsewhere each
    time), the planes' is made once and is not the matrix's; every result is the restatement's and nothing is withheld."""
    from tests.test_gpu_binding_decomposition import check as check_planes
    from tests.test_gpu_binding_decomposition import reference as plane_reference
    s = systems("trpcage")
    sets, S = residues("trpcage")
    mod3 = np.arange(s.n) % 3
    ligand = list(range(16))
    b = _binding(s, ligand, sets, S)
    planes = plane_reference(s, ligand, "file", s.pos)
    check(b.pair_matrix(s.pos), reference(s, ligand, sets, S, "file", s.pos), what="host, 20 sets")
    check_planes(b.decompose(s.pos), planes, what="host, after 20 sets")
    b.set_atom_sets(mod3)
    check(b.pair_matrix(s.pos), reference(s, ligand, mod3, 3, "file", s.pos), what="host, 3 sets")
    check_planes(b.decompose(s.pos), planes, what="host, after 3 sets")
    b.set_atom_sets(sets, S)
    check(b.pair_matrix(s.pos), reference(s, ligand, sets, S, "file", s.pos), what="host, 20 sets again")
    assert b.finish() == 0 and b.withheld() == []


def test_update_parameters_keeps_the_partition(gpu_required, systems, five_groups):
    s = systems("trpcage")
    sets, S = residues("trpcage")
    ligand = list(range(16))
    force = P.AGBNPForce.from_arrays(*s.params(), version=1)
    b = P.BindingEnergy(force, ligand, device=0)
    b.set_atom_sets(sets)
    check(b.pair_matrix(s.pos), reference(s, ligand, sets, S, "file", s.pos), what="before the update")
    for i in range(s.n):
        r, g, a, q, h = force.getParticleParameters(i)
        force.setParticleParameters(i, r, g, a, 0.5 * q, h)
    b.copyParametersToContext(force)
    assert b.num_atom_sets() == S and [b.member(m).num_atom_sets() for m in range(3)] == [S] * 3
    halved = (s.radius, s.gamma, s.alpha, 0.5 * s.charge, s.ishydrogen)
    check(b.pair_matrix(s.pos), reference(s, ligand, sets, S, "halved", s.pos, params=halved), what="halved charges")


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------
def test_without_a_partition_the_calls_are_refused(gpu_required, systems, five_groups):
    s = systems("trpcage")
    b = _binding(s, list(range(16)))
    assert b.num_atom_sets() == 0
    with pytest.raises(P.OpenMMException, match="no partition has been set"):
        b.pair_matrix(s.pos)
    with pytest.raises(P.OpenMMException, match="no partition has been set"):
        b.pair_matrix_device(1, 2)
    assert b.finish() == 0
    e, u = b.energy(s.pos, 0.35)  # (the binding goes on)
    assert np.isfinite(e) and np.isfinite(u)


def test_pair_matrix_device_refuses_a_stream_capture(gpu_required, systems, five_groups):
    """Inside a capture the call is refused before the gather: nothing is launched, the capture ends cleanly and replays, no
    evaluation is logged, and the binding goes on."""
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    sets, S = residues("trpcage")
    ligand = list(range(16))
    b = _binding(s, ligand, sets)
    b.pair_matrix(s.pos)
    buf = Buffers(torch, s.n, S)
    buf.load(s.jittered(1))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        buf.u.fill_(1.0)
        with pytest.raises(P.OpenMMException, match="captur"):
            b.pair_matrix_device(buf.pos.data_ptr(), buf.matrix.data_ptr(), buf.u.data_ptr(), torch.cuda.current_stream().cuda_stream)
    buf.u.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert buf.u.item() == 1.0 and not buf.matrix.any().item()
    assert b.finish(buf.stream) == 0
    buf.u.zero_()
    buf.evaluate(b)
    assert b.finish(buf.stream) == 0
    check(buf.result(), reference(s, ligand, sets, S, "jitter1", s.jittered(1)), what="after the refusal")


def test_the_host_form_repeats_a_withheld_evaluation(gpu_required, systems, five_groups):
    s = systems("trpcage")
    sets, S = residues("trpcage")
    ligand = list(range(16))
    b = _binding(s, ligand, sets)
    check(b.pair_matrix(s.pos), reference(s, ligand, sets, S, "file", s.pos), what="host")
    moved = s.jittered(6) + np.array([0.0, 0.1, 0.0])  # every atom jumps: all three members are withheld once, repeated inside
    check(b.pair_matrix(moved), reference(s, ligand, sets, S, "jitter6_moved", moved), what="host across a jump")
    assert b.finish() == 0 and b.withheld() == []


# ---- 8. a protein ---------------------------------------------------------------------------------------------------------------
def test_1dwc_residues_and_a_30_atom_ligand(gpu_required, systems, five_groups):
    """258 residues, 2145 tiles in the complex; the last 30 atoms as the ligand."""
    s = systems("1dwc")
    sets, S = residues("1dwc")
    ligand = list(range(s.n - 30, s.n))
    b = _binding(s, ligand, sets)
    d, u = b.pair_matrix(s.pos)
    check((d, u), reference(s, ligand, sets, S, "file", s.pos), what="1dwc")
    assert np.abs(d - d.T).max() < SAME
