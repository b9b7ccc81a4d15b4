"""GPU box: binding-energy evaluations (include/agbnp_hip.h: agbnp_hip_binding_*) -- the complex, its receptor and
its ligand in one call, every output gated on all three verdicts on the device.  The reference is the NumPy combination of three
CPU oracles (tests/binding_restatement.py, pinned on the CPU by tests/test_binding_restatement.py); the three oracles of a
partition are made once and an evaluation of a geometry is shared (REFS).

Tolerances: the project's TIGHT = 1e-7 per member evaluation and the weights of the combination --
    forces   TIGHT (|lam| + |1 - lam|)            E_lam   TIGHT (|lam| + 2 |1 - lam|)            u   3 TIGHT
the energies on energy_close's scale (max(1, 1e-3 |E|)) taken at the largest of the three |E|."""
import os
import subprocess

import numpy as np
import pytest

import openmm_agbnp_plugin_amd as P
from tests.binding_restatement import BindingRestatement, combine
from tests.edge_systems import edge_systems
from tests.gpu_helpers import SAME, TIGHT
from tests.gpu_helpers import energy_close as _energy_close
from tests.gpu_helpers import five_groups  # noqa: F401

pytestmark = pytest.mark.gpu

RESTATEMENTS = {}
REFS = {}
LAMBDAS = (0.0, 0.35, 1.0, 1.5)


def _key(s, ligand, version, cutoff, ptag):
    return (s.name, tuple(sorted(int(a) for a in ligand)), version, cutoff, ptag)


def reference(s, ligand, tag, pos, version=1, cutoff=None, params=None, ptag="file"):
    """((E_RL, E_R, E_L), F_RL, F_own) of the restatement at `pos`, once per partition and geometry tag."""
    key = _key(s, ligand, version, cutoff, ptag)
    if key not in RESTATEMENTS:
        RESTATEMENTS[key] = BindingRestatement(params or s.params(), ligand, version=version, cutoff=cutoff)
    if key + (tag,) not in REFS:
        energies, f_rl, f_own = RESTATEMENTS[key].evaluate(pos)
        f_rl.setflags(write=False)
        f_own.setflags(write=False)
        REFS[key + (tag,)] = (energies, f_rl, f_own)
    return REFS[key + (tag,)]


def _binding(s, ligand, version=1, mode="reference", cutoff=None):
    force = P.AGBNPForce.from_arrays(*s.params(), version=version)
    if cutoff is not None:
        force.setNonbondedMethod(P.AGBNPForce.CutoffNonPeriodic)
        force.setCutoffDistance(cutoff)
    return P.BindingEnergy(force, ligand, device=0, mode=mode)


def check(got, ref, lam, count=1, fill=(0.0, 0.0, 0.0), what=""):
    """got = (E_lam, u, F_lam) as the engine gave them -- `count` evaluations of this reference added to `fill` -- against the
    restatement, within the tolerances of the module's docstring (times count)."""
    energies, f_rl, f_own = ref
    e_ref, u_ref, f_ref = combine(energies, f_rl, f_own, lam)
    unit = max(1.0, 1e-3 * max(abs(x) for x in energies))
    e, u, f = got
    de, du = abs(e - fill[0] - count * e_ref), abs(u - fill[1] - count * u_ref)
    df = float(np.abs(np.asarray(f).reshape(-1, 3) - fill[2] - count * f_ref).max())
    print(f"binding {what} lam={lam}: |dE_lam| {de:.2e}  |du| {du:.2e}  max|dF| {df:.2e}  (scale {unit:.3f})")
    assert df < count * TIGHT * (abs(lam) + abs(1.0 - lam)), f"forces differ by {df:.3e}"
    assert de < count * TIGHT * (abs(lam) + 2.0 * abs(1.0 - lam)) * unit, f"E_lambda differs by {de:.3e}"
    assert du < count * 3.0 * TIGHT * unit, f"u differs by {du:.3e}"


class Buffers:
    """The caller's device buffers of a binding: positions, forces, E_lam and u (torch tensors), pre-filled."""

    def __init__(self, torch, n, fill=(0.0, 0.0, 0.0)):
        dev = torch.device("cuda:0")
        self.torch, self.fill = torch, fill
        self.pos = torch.zeros((n, 3), dtype=torch.float64, device=dev)
        self.ene = torch.full((1,), fill[0], dtype=torch.float64, device=dev)
        self.u = torch.full((1,), fill[1], dtype=torch.float64, device=dev)
        self.frc = torch.full((n, 3), fill[2], dtype=torch.float64, device=dev)
        self.stream = torch.cuda.current_stream().cuda_stream
        torch.cuda.synchronize()  # (the fills ran on torch's stream; the evaluations run on the binding's)

    def load(self, geom):
        self.pos.copy_(self.torch.tensor(np.asarray(geom), dtype=self.torch.float64))
        self.torch.cuda.synchronize()

    def execute(self, b, lam):
        b.execute_device(self.pos.data_ptr(), lam, self.frc.data_ptr(), self.ene.data_ptr(), self.u.data_ptr(), self.stream)

    def energy(self, b, lam):
        b.energy_device(self.pos.data_ptr(), lam, self.ene.data_ptr(), self.u.data_ptr(), self.stream)

    def result(self):
        return self.ene.item(), self.u.item(), self.frc.cpu().numpy()

    def snapshot(self):
        return self.ene.clone(), self.u.clone(), self.frc.clone()

    def unchanged_since(self, snap):
        return all(self.torch.equal(a, b) for a, b in zip((self.ene, self.u, self.frc), snap))


def _moved(s, atom, by=0.1):
    pos = s.pos.copy()
    pos[atom, 0] += by
    return pos


# ---- 1. parity with the restatement ----------------------------------------------------------------------------------
PARITY = {  # name -> (system, ligand atoms, version, geometries)
    "trpcage_0_15_v1": ("trpcage", range(0, 16), 1, 3),
    "trpcage_100_129_v0": ("trpcage", range(100, 130), 0, 3),
    "fixture264_200_263": ("fixture264", range(200, 264), 1, 3),
    "1dwc_4122_4151": ("1dwc", range(4122, 4152), 1, 1),
}


@pytest.mark.parametrize("case", sorted(PARITY))
def test_parity_with_the_restatement(gpu_required, systems, five_groups, case):
    name, ligand, version, geometries = PARITY[case]
    s = systems(name)
    b = _binding(s, ligand, version=version)
    assert b.ligand_atoms.tolist() == list(ligand) and len(b.receptor_atoms) == s.n - len(ligand)
    for step in range(geometries):
        pos = s.jittered(step)
        ref = reference(s, ligand, f"jitter{step}", pos, version=version)
        for lam in LAMBDAS:
            check(b.execute(pos, lam), ref, lam, what=f"{case} step {step}")
        e, u = b.energy(pos, 0.35)
        check((e, u, combine(*ref, 0.35)[2]), ref, 0.35, what=f"{case} step {step} energy()")
    assert b.finish() == 0 and b.withheld() == []


# ---- 2. index maps and block edges -----------------------------------------------------------------------------------
EDGES = {  # name -> (system, ligand atoms or "heavy", version)
    "size_1_33_heavy_v0": ("size_1_33", "heavy", 0),
    "size_1_33_heavy_v1": ("size_1_33", "heavy", 1),
    "size_129_257_every_third": ("size_129_257", range(0, 257, 3), 1),
    "size_129_257_atom_0": ("size_129_257", [0], 1),
    "size_129_257_atom_256": ("size_129_257", [256], 1),
    "size_257_513_last_block": ("size_257_513", range(256, 513), 1),
}


@pytest.mark.parametrize("case", sorted(EDGES))
def test_index_maps_and_block_edges(gpu_required, five_groups, case):
    """A receptor without a heavy atom; a ligand strewn over the complex; the first and the last atom alone (the last one is a
    block of its own); a ligand that is the second half and ends one atom into a new 256-thread block."""
    name, ligand, version = EDGES[case]
    s = edge_systems()[name]
    if isinstance(ligand, str):
        ligand = np.flatnonzero(s.ishydrogen == 0).tolist()
        assert len(ligand) == 1
    ligand = list(ligand)
    b = _binding(s, ligand, version=version)
    ref = reference(s, ligand, "file", s.pos, version=version)
    got = b.execute(s.pos, 0.35)
    check(got, ref, 0.35, what=case)
    if case == "size_1_33_heavy_v0":
        assert abs(got[1]) < 3.0 * TIGHT  # (u = 0: the receptor is 32 hydrogens)
    e, u = b.energy(s.pos, 0.35)
    check((e, u, got[2]), ref, 0.35, what=case + " energy()")


def test_the_order_of_the_ligand_list_does_not_matter(gpu_required, systems, five_groups):
    s = systems("trpcage")
    down = _binding(s, list(range(15, -1, -1)))
    up = _binding(s, list(range(16)))
    assert down.ligand_atoms.tolist() == up.ligand_atoms.tolist() == list(range(16))
    assert down.receptor_atoms.tolist() == up.receptor_atoms.tolist() == list(range(16, s.n))
    got_down, got_up = down.execute(s.pos, 0.35), up.execute(s.pos, 0.35)
    check(got_down, reference(s, range(16), "file", s.pos), 0.35, what="descending list")
    _energy_close(got_down[0], got_up[0], SAME)
    _energy_close(got_down[1], got_up[1], SAME)
    assert np.abs(got_down[2] - got_up[2]).max() < SAME


# ---- 3. the ends of lambda against twins -----------------------------------------------------------------------------
def test_the_ends_of_lambda_are_a_twin_context(gpu_required, systems, five_groups):
    """lambda = 1: forces and energy of a separate context of the complex through execute_device at the same positions;
    lambda = 0: the receptor atoms' forces are a separate receptor context's."""
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    ligand = list(range(16))
    b = _binding(s, ligand)
    pos = s.jittered(1)
    buf = Buffers(torch, s.n)
    buf.load(pos)
    buf.execute(b, 1.0)
    assert b.finish(buf.stream) == 0
    e1, u1, f1 = buf.result()

    def twin(system, geom):
        k = P.HipCalcAGBNPForceKernel(device=0)
        k.initialize(P.AGBNPForce.from_arrays(*system.params(), version=1))
        t = Buffers(torch, system.n)
        t.load(geom)
        k.execute_device(t.pos.data_ptr(), t.frc.data_ptr(), t.ene.data_ptr(), t.stream)
        assert k.finish(t.stream) == 0
        return t.ene.item(), t.frc.cpu().numpy()

    e_twin, f_twin = twin(s, pos)
    _energy_close(e1, e_twin, SAME)
    assert np.abs(f1 - f_twin).max() < SAME
    buf = Buffers(torch, s.n)
    buf.load(pos)
    buf.execute(b, 0.0)
    assert b.finish(buf.stream) == 0
    e0, u0, f0 = buf.result()
    receptor = b.receptor_atoms
    e_r, f_r = twin(s.subset(receptor), pos[receptor])
    assert np.abs(f0[receptor] - f_r).max() < SAME
    _energy_close(u0, u1, SAME)
    _energy_close(e1 - u1, e0, SAME)  # (E_1 - u = E_R + E_L = E_0)
    check((e0, u0, f0), reference(s, ligand, "jitter1", pos), 0.0, what="lambda 0")


# ---- 4. the device call adds -----------------------------------------------------------------------------------------
def test_the_device_call_adds_and_takes_null_scalars(gpu_required, systems, five_groups):
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    ligand = list(range(16))
    b = _binding(s, ligand)
    pos = s.jittered(1)
    ref = reference(s, ligand, "jitter1", pos)
    fill = (2.0, 3.0, 1.0)
    buf = Buffers(torch, s.n, fill)
    buf.load(pos)
    pos0 = buf.pos.clone()
    buf.execute(b, 0.35)
    buf.execute(b, 0.35)
    no_e, no_u = Buffers(torch, s.n), Buffers(torch, s.n)
    b.execute_device(buf.pos.data_ptr(), 0.35, no_e.frc.data_ptr(), None, no_e.u.data_ptr(), buf.stream)
    b.execute_device(buf.pos.data_ptr(), 0.35, no_u.frc.data_ptr(), no_u.ene.data_ptr(), None, buf.stream)
    b.execute_device(buf.pos.data_ptr(), 0.35, no_u.frc.data_ptr(), None, None, buf.stream)
    assert b.finish(buf.stream) == 0, b.withheld()
    check(buf.result(), ref, 0.35, count=2, fill=fill, what="two into filled buffers")
    e_ref, u_ref, _ = combine(*ref, 0.35)
    check((e_ref, no_e.u.item(), no_e.frc.cpu().numpy()), ref, 0.35, what="d_energy NULL")
    assert no_e.ene.item() == 0.0 and no_u.u.item() == 0.0
    check((no_u.ene.item(), 2.0 * u_ref, no_u.frc.cpu().numpy()), ref, 0.35, count=2, fill=(-e_ref, 0.0, 0.0), what="d_binding_energy NULL")
    assert torch.equal(buf.pos, pos0)
    with pytest.raises(P.OpenMMException):
        b.energy_device(buf.pos.data_ptr(), 0.35, None, None, buf.stream)
    with pytest.raises(P.OpenMMException):
        b.execute_device(buf.pos.data_ptr(), float("nan"), buf.frc.data_ptr(), None, None, buf.stream)
    assert b.finish(buf.stream) == 0


# ---- 5. energy-only --------------------------------------------------------------------------------------------------
def test_the_energy_only_form_writes_no_force(gpu_required, systems, five_groups):
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    ligand = list(range(16))
    b = _binding(s, ligand)
    pos = s.jittered(1)
    full = Buffers(torch, s.n)
    full.load(pos)
    full.execute(b, 0.35)
    assert b.finish(full.stream) == 0
    e_full, u_full, _ = full.result()
    sentinel = -123.456
    full.frc.fill_(sentinel)  # (the buffer the full call wrote)
    only = Buffers(torch, s.n, (0.0, 0.0, sentinel))
    only.load(pos)
    only.energy(b, 0.35)
    assert [int(b.member(m).scalar("last_evaluation_kind")) in (1, 2) for m in range(3)] == [True] * 3
    assert b.finish(only.stream) == 0
    torch.cuda.synchronize()
    _energy_close(only.ene.item(), e_full, SAME)
    _energy_close(only.u.item(), u_full, SAME)
    assert (only.frc == sentinel).all().item() and (full.frc == sentinel).all().item()
    full.execute(b, 0.35)  # (and a full call behind it finds the binding's buffers clean)
    assert b.finish(full.stream) == 0
    assert [int(b.member(m).scalar("last_evaluation_kind")) for m in range(3)] == [0, 0, 0]
    check((full.ene.item() - e_full, full.u.item() - u_full, full.frc.cpu().numpy() - sentinel), reference(s, ligand, "jitter1", pos), 0.35,
          what="full behind energy-only")


# ---- 6. all or nothing -----------------------------------------------------------------------------------------------
def test_a_jump_of_a_ligand_atom_withholds_everything_and_a_hint_prevents_it(gpu_required, systems, five_groups):
    """The moved atom makes the complex and the ligand jump; the receptor's evaluation is complete, its forces are in the
    binding's own buffer -- and must neither reach the caller nor stay there for the repeat."""
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    ligand = list(range(16))
    b = _binding(s, ligand)
    fill = (2.0, 3.0, 1.0)
    buf = Buffers(torch, s.n, fill)
    buf.load(s.pos)
    buf.execute(b, 0.35)
    assert b.finish(buf.stream) == 0
    assert int(b.member(0).scalar("launches")) == 5
    heavy_ligand = [a for a in ligand if s.ishydrogen[a] == 0]
    moved = _moved(s, heavy_ligand[len(heavy_ligand) // 2])
    buf.load(moved)
    torch.cuda.synchronize()
    snap = buf.snapshot()
    buf.execute(b, 0.35)
    assert b.finish(buf.stream) == 1 and b.withheld() == [0]
    torch.cuda.synchronize()
    assert buf.unchanged_since(snap)  # bit for bit
    assert int(b.member(0).scalar("overflow_kinds")) & 16 and int(b.member(2).scalar("overflow_kinds")) & 16
    assert int(b.member(1).scalar("overflow_kinds")) == 0  # (the receptor was complete)
    rep = Buffers(torch, s.n, fill)
    rep.load(moved)
    rep.execute(b, 0.35)  # the repeat
    assert b.finish(rep.stream) == 0 and b.withheld() == []
    check(rep.result(), reference(s, ligand, "moved_ligand", moved), 0.35, fill=fill, what="repeat after a ligand jump")
    # with the hint nothing is withheld
    moved2 = _moved(s, heavy_ligand[0], -0.1)
    fresh = Buffers(torch, s.n)
    fresh.load(moved2)
    b.expect_jump()
    fresh.execute(b, 0.35)
    assert b.finish(fresh.stream) == 0, b.withheld()
    check(fresh.result(), reference(s, ligand, "moved_ligand2", moved2), 0.35, what="behind the hint")


def test_a_jump_of_a_receptor_atom_leaves_nothing_of_the_ligand_behind(gpu_required, systems, five_groups):
    """The ligand member is complete while the complex and the receptor are withheld: outputs untouched, and the repeat shows that
    the binding's own buffers were cleared after the withheld evaluation.  The energy-only form is gated the same way."""
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    ligand = list(range(16))
    b = _binding(s, ligand)
    buf = Buffers(torch, s.n, (2.0, 3.0, 1.0))
    buf.load(s.pos)
    b.expect_jump()
    buf.energy(b, 0.35)
    assert b.finish(buf.stream) == 0
    heavy_receptor = np.array([a for a in b.receptor_atoms if s.ishydrogen[a] == 0])
    gap = np.linalg.norm(s.pos[heavy_receptor][:, None, :] - s.pos[ligand][None, :, :], axis=-1).min(axis=1)
    far = int(heavy_receptor[np.argmax(gap)])
    moved = _moved(s, far)
    buf.load(moved)
    torch.cuda.synchronize()
    snap = buf.snapshot()
    buf.execute(b, 0.35)
    assert b.finish(buf.stream) == 1 and b.withheld() == [0]
    torch.cuda.synchronize()
    assert buf.unchanged_since(snap)
    assert int(b.member(2).scalar("overflow_kinds")) == 0  # (the ligand was complete)
    fresh = Buffers(torch, s.n)
    fresh.load(moved)
    fresh.execute(b, 0.35)  # the repeat
    assert b.finish(fresh.stream) == 0
    check(fresh.result(), reference(s, ligand, "moved_receptor", moved), 0.35, what="repeat after a receptor jump")
    # the energy-only form across the next jump
    back = Buffers(torch, s.n, (2.0, 3.0, 1.0))
    back.load(s.pos)
    torch.cuda.synchronize()
    snap = back.snapshot()
    back.energy(b, 0.35)
    assert b.finish(back.stream) == 1 and b.withheld() == [0]
    torch.cuda.synchronize()
    assert back.unchanged_since(snap)
    back.energy(b, 0.35)
    assert b.finish(back.stream) == 0
    e_ref, u_ref, f_ref = combine(*reference(s, ligand, "file", s.pos), 0.35)
    check((back.ene.item(), back.u.item(), f_ref + 1.0), reference(s, ligand, "file", s.pos), 0.35, fill=(2.0, 3.0, 1.0), what="energy-only repeat")


# ---- 7. queueing and the steady state --------------------------------------------------------------------------------
def test_twenty_queued_evaluations_and_a_steady_argument_block(gpu_required, systems, five_groups):
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    ligand = list(range(16))
    b = _binding(s, ligand)
    steps = 20
    geoms = [s.jittered(step) for step in range(steps)]
    walk = torch.tensor(np.stack(geoms), dtype=torch.float64, device=torch.device("cuda:0"))
    buf = Buffers(torch, s.n)
    torch.cuda.synchronize()
    # a stream of the caller's own: the copies into the ONE position buffer and the evaluations are ordered on it (torch's default
    # stream has the handle 0, which the library takes for "the complex's own stream" -- copies on it would not be ordered)
    side = torch.cuda.Stream()
    buf.stream = side.cuda_stream
    assert buf.stream != 0
    writes = None
    with torch.cuda.stream(side):
        for k in range(steps):
            buf.pos.copy_(walk[k])
            buf.execute(b, 0.35)
            if k == 1:
                writes = [int(b.member(m).scalar("group_block_writes")) for m in range(3)]
    assert [int(b.member(m).scalar("group_members")) for m in range(3)] == [3, 3, 3]
    assert b.finish(buf.stream) == 0, b.withheld()
    torch.cuda.synchronize()
    assert [int(b.member(m).scalar("group_block_writes")) for m in range(3)] == writes
    total = [0.0, 0.0, np.zeros((s.n, 3))]
    worst = 0.0
    for step, pos in enumerate(geoms):
        ref = reference(s, ligand, f"jitter{step}", pos)
        e, u, f = combine(*ref, 0.35)
        total[0] += e
        total[1] += u
        total[2] += f
        worst = max(worst, max(abs(x) for x in ref[0]))
    e, u, f = buf.result()
    unit = max(1.0, 1e-3 * worst)
    de, du, df = abs(e - total[0]), abs(u - total[1]), float(np.abs(f - total[2]).max())
    print(f"20 queued: |dE_lam| {de:.2e}  |du| {du:.2e}  max|dF| {df:.2e}")
    assert df < steps * TIGHT and de < steps * TIGHT * (0.35 + 2 * 0.65) * unit and du < steps * 3 * TIGHT * unit


# ---- 8. modes --------------------------------------------------------------------------------------------------------
def test_fast_mode_with_a_cutoff(gpu_required, systems, five_groups):
    s = systems("trpcage")
    ligand = list(range(16))
    b = _binding(s, ligand, mode="fast", cutoff=1.0)
    ref = reference(s, ligand, "file", s.pos, cutoff=1.0)
    for lam in (0.35, 1.0):
        check(b.execute(s.pos, lam), ref, lam, what="fast mode")
    plain = reference(s, ligand, "file", s.pos)
    assert abs(ref[0][0] - plain[0][0]) > 1e-3  # (the cutoff truncates something: another reference)


def test_deterministic_mode_is_bit_identical(gpu_required, systems, five_groups):
    s = systems("trpcage")
    ligand = list(range(16))
    b = _binding(s, ligand, mode="deterministic")
    e1, u1, f1 = b.execute(s.pos, 0.35)
    e2, u2, f2 = b.execute(s.pos, 0.35)
    assert e1 == e2 and u1 == u2 and np.array_equal(f1, f2)
    check((e1, u1, f1), reference(s, ligand, "file", s.pos), 0.35, what="deterministic mode")
    b.set_mode("reference")
    check(b.execute(s.pos, 0.35), reference(s, ligand, "file", s.pos), 0.35, what="back in the reference mode")


def test_members_that_run_their_own_launches(gpu_required, systems, monkeypatch):
    monkeypatch.setenv("AGBNP_HIP_FIVE_LAUNCHES", "1")
    monkeypatch.setenv("AGBNP_HIP_GROUP_LAUNCHES", "0")
    s = systems("trpcage")
    ligand = list(range(16))
    b = _binding(s, ligand)
    for step in range(2):
        pos = s.jittered(step)
        check(b.execute(pos, 0.35), reference(s, ligand, f"jitter{step}", pos), 0.35, what="group launches off")
    assert [int(b.member(m).scalar("group_members")) for m in range(3)] == [0, 0, 0]


# ---- 9. parameters, capture, host entries ----------------------------------------------------------------------------
def test_halved_ligand_charges(gpu_required, systems, five_groups):
    s = systems("trpcage")
    ligand = list(range(16))
    force = P.AGBNPForce.from_arrays(*s.params(), version=1)
    b = P.BindingEnergy(force, ligand)
    before = b.execute(s.pos, 0.35)
    check(before, reference(s, ligand, "file", s.pos), 0.35, what="before the update")
    charge = s.charge.copy()
    charge[ligand] *= 0.5
    for i in ligand:
        r, g, a, q, h = force.getParticleParameters(i)
        force.setParticleParameters(i, r, g, a, 0.5 * q, h)
    b.copyParametersToContext(force)
    halved = (s.radius, s.gamma, s.alpha, charge, s.ishydrogen)
    ref = reference(s, ligand, "file", s.pos, params=halved, ptag="halved_ligand")
    after = b.execute(s.pos, 0.35)
    check(after, ref, 0.35, what="halved ligand charges")
    assert abs(after[1] - before[1]) > 1e-3


def test_the_device_calls_refuse_a_stream_capture(gpu_required, systems, five_groups):
    """Inside a capture both calls fail with INVALID_ARGUMENT, launch nothing, and the capture ends cleanly and replays."""
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    ligand = list(range(16))
    b = _binding(s, ligand)
    buf = Buffers(torch, s.n)
    buf.load(s.pos)
    buf.execute(b, 0.35)
    assert b.finish(buf.stream) == 0
    first = buf.result()
    marker = torch.zeros((1,), dtype=torch.float64, device=torch.device("cuda:0"))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        marker.fill_(1.0)
        stream = torch.cuda.current_stream().cuda_stream
        with pytest.raises(P.OpenMMException, match="captur"):
            b.execute_device(buf.pos.data_ptr(), 0.35, buf.frc.data_ptr(), buf.ene.data_ptr(), buf.u.data_ptr(), stream)
        with pytest.raises(P.OpenMMException, match="captur"):
            b.energy_device(buf.pos.data_ptr(), 0.35, buf.ene.data_ptr(), buf.u.data_ptr(), stream)
    marker.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert marker.item() == 1.0
    after = buf.result()
    assert after[0] == first[0] and after[1] == first[1] and np.array_equal(after[2], first[2])  # nothing was launched
    buf.execute(b, 0.35)  # the binding goes on as before
    assert b.finish(buf.stream) == 0
    check(buf.result(), reference(s, ligand, "file", s.pos), 0.35, count=2, what="behind the refused capture")


def test_the_host_entries_repeat_and_carry_withheld_evaluations(gpu_required, systems, five_groups):
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    ligand = list(range(16))
    b = _binding(s, ligand)
    check(b.execute(s.pos, 0.35), reference(s, ligand, "file", s.pos), 0.35, what="host, file")
    heavy = np.flatnonzero(s.ishydrogen == 0)
    moved = _moved(s, int(heavy[len(heavy) // 2]))
    check(b.execute(moved, 0.35), reference(s, ligand, "moved_host", moved), 0.35, what="host across a jump")
    e, u = b.energy(s.pos, 0.35)
    check((e, u, combine(*reference(s, ligand, "file", s.pos), 0.35)[2]), reference(s, ligand, "file", s.pos), 0.35, what="host energy across a jump")
    # a device evaluation that is withheld and still unfinished when a host entry harvests the log: the next finish reports it
    buf = Buffers(torch, s.n, (2.0, 3.0, 1.0))
    buf.load(moved)
    torch.cuda.synchronize()
    snap = buf.snapshot()
    buf.execute(b, 0.35)
    check(b.execute(s.pos, 0.35), reference(s, ligand, "file", s.pos), 0.35, what="host behind an unfinished device call")
    assert b.finish(buf.stream) == 1 and b.withheld() == [0]
    torch.cuda.synchronize()
    assert buf.unchanged_since(snap)


def test_cpp_mirror_runs_a_binding(gpu_required, systems, five_groups, tmp_path):
    """tests/cxx/TestHipBinding.cpp through cpp/AGBNPForce.h."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(root, "openmm_agbnp_plugin_amd")
    exe = str(tmp_path / "TestHipBinding")
    subprocess.run(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", os.path.join(root, "tests", "cxx", "TestHipBinding.cpp"),
                    "-o", exe, os.path.join(libdir, "libagbnp_hip.so"), "-L/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{libdir}",
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    x = systems("trpcage")
    path = tmp_path / "trpcage.txt"
    r, g, a, q, h = x.params()
    np.savetxt(path, np.column_stack([r, g, a, q, np.asarray(h, dtype=float), x.pos]), fmt="%.17g")
    out = subprocess.run([exe, str(path), "16"], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
