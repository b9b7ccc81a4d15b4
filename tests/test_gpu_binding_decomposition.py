"""GPU box: per-atom decomposition of a binding energy (include/agbnp_hip.h: agbnp_hip_binding_decompose_device / _host; DESIGN.md
s.4q) -- D[t][i] = T_RL[t][i] - T_own[t][own(i)] from ONE decomposition group over the complex, its receptor and its ligand, gated
on all three verdicts on the device.  The reference is tests/binding_decomposition_restatement.py (pinned on the CPU by
tests/test_binding_decomposition_restatement.py); the restatement of a partition at a geometry is computed once and shared (REFS).

Tolerances: every one of the 4 N terms within 2 TIGHT (a difference of two member terms, TIGHT = 1e-7 each), u within 3 TIGHT on
energy_close's scale (max(1, 1e-3 |E|)), as tests/test_gpu_binding.py has it; `count` evaluations added to a buffer, times count."""
import os
import subprocess

import numpy as np
import pytest

import openmm_agbnp_plugin_amd as P
from tests.binding_decomposition_restatement import restate
from tests.binding_restatement import restate as restate_binding
from tests.edge_systems import edge_systems
from tests.gpu_helpers import SAME, TIGHT
from tests.gpu_helpers import five_groups  # noqa: F401

pytestmark = pytest.mark.gpu
SENTINEL = -1234.5678
REFS = {}
WORST = [0.0]  # the worst |term - restatement| this file has seen (printed by every comparison)


def reference(s, ligand, tag, pos, version=1, cutoff=None):
    """(D[4, N], u, scale) of the restatement at `pos`, once per partition and geometry tag."""
    key = (s.name, tuple(sorted(int(a) for a in ligand)), version, cutoff, tag)
    if key not in REFS:
        d, u = restate(s.params(), ligand, pos, version=version, cutoff=cutoff)
        energies = restate_binding(s.params(), ligand, pos, 0.35, version=version, cutoff=cutoff)[3]
        d.setflags(write=False)
        REFS[key] = (d, u, max(1.0, 1e-3 * max(abs(x) for x in energies)))
    return REFS[key]


def _binding(s, ligand, version=1, mode="reference", cutoff=None):
    force = P.AGBNPForce.from_arrays(*s.params(), version=version)
    if cutoff is not None:
        force.setNonbondedMethod(P.AGBNPForce.CutoffNonPeriodic)
        force.setCutoffDistance(cutoff)
    return P.BindingEnergy(force, ligand, device=0, mode=mode)


def check(got, ref, count=1, fill=(0.0, 0.0), what=""):
    """got = (terms[4, N], u) as the engine gave them -- `count` evaluations of this reference added to `fill`."""
    d_ref, u_ref, unit = ref
    terms, u = got
    terms = np.asarray(terms).reshape(4, -1)
    worst = np.abs(terms - fill[0] - count * d_ref).max(axis=1)
    du = abs(u - fill[1] - count * u_ref)
    WORST[0] = max(WORST[0], float(worst.max()) / count)
    print(f"binding decomposition {what}: worst |term - restatement| per plane {worst}  |du| {du:.2e}  (scale {unit:.3f}; "
          f"file so far {WORST[0]:.3e})")
    assert worst.max() < count * 2.0 * TIGHT, f"terms differ by {worst} (planes cavity, vdw, gb_self, gb_pair)"
    assert du < count * 3.0 * TIGHT * unit, f"u differs by {du:.3e}"


class Buffers:
    """The caller's device buffers: positions, the planes [4, N] and u (torch tensors), pre-filled."""

    def __init__(self, torch, n, fill=(0.0, 0.0)):
        dev = torch.device("cuda:0")
        self.torch, self.fill = torch, fill
        self.pos = torch.zeros((n, 3), dtype=torch.float64, device=dev)
        self.terms = torch.full((4, n), fill[0], dtype=torch.float64, device=dev)
        self.u = torch.full((1,), fill[1], dtype=torch.float64, device=dev)
        self.stream = torch.cuda.current_stream().cuda_stream

    def load(self, geom):
        self.pos.copy_(self.torch.tensor(np.asarray(geom), dtype=self.torch.float64))

    def decompose(self, b, with_u=True):
        b.decompose_device(self.pos.data_ptr(), self.terms.data_ptr(), self.u.data_ptr() if with_u else None, self.stream)

    def result(self):
        return self.terms.cpu().numpy(), self.u.item()

    def snapshot(self):
        return self.terms.clone(), self.u.clone()

    def unchanged_since(self, snap):
        return all(self.torch.equal(a, b) for a, b in zip((self.terms, self.u), snap))


def _moved(s, atom, by=0.1):
    pos = s.pos.copy()
    pos[atom, 0] += by
    return pos


# ---- 1. parity with the restatement, index maps and block edges --------------------------------------------------------------
PARTITIONS = {  # name -> (system, ligand atoms, version)
    "trpcage_0_15": ("trpcage", range(0, 16), 1),
    "trpcage_every_third": ("trpcage", range(0, 272, 3), 1),
    "fixture264_200_263_v0": ("fixture264", range(200, 264), 0),
    "fixture264_200_263_v1": ("fixture264", range(200, 264), 1),
    "size_257_513_last_257": ("size_257_513", range(256, 513), 1),
    "size_257_513_atom_256": ("size_257_513", [256], 1),
}


@pytest.mark.parametrize("case", sorted(PARTITIONS))
def test_parity_with_the_restatement(gpu_required, systems, five_groups, case):
    """A contiguous ligand; a ligand strewn over the complex (every index of both maps off the diagonal); both versions; a ligand
    that is the second half and ends one atom into a new 256-thread block of the combine launch and a new 64-atom block of the
    plane launch; that one atom alone.  The host form and the device form; the terms sum to the u of energy_device."""
    torch = pytest.importorskip("torch")
    name, ligand, version = PARTITIONS[case]
    s = edge_systems()[name] if name.startswith("size_") else systems(name)
    ligand = list(ligand)
    b = _binding(s, ligand, version=version)
    ref = reference(s, ligand, "file", s.pos, version=version)
    terms, u = b.decompose(s.pos)
    check((terms, u), ref, what=case + " host")
    if version == 0:
        assert (terms[1:] == 0.0).all()
    buf = Buffers(torch, s.n)
    buf.load(s.pos)
    buf.decompose(b)
    e_word = torch.zeros((2,), dtype=torch.float64, device=buf.pos.device)
    b.energy_device(buf.pos.data_ptr(), 0.35, e_word[0:1].data_ptr(), e_word[1:2].data_ptr(), buf.stream)
    assert b.finish(buf.stream) == 0 and b.withheld() == []
    got = buf.result()
    check(got, ref, what=case + " device")
    u_energy = e_word[1].item()
    print(f"{case}: sum D {got[0].sum()!r}  u (decompose) {got[1]!r}  u (energy_device) {u_energy!r}")
    assert abs(got[0].sum() - u_energy) < 3.0 * TIGHT * ref[2]
    assert abs(got[1] - u_energy) < SAME * ref[2]


def test_the_order_of_the_ligand_list_does_not_matter(gpu_required, systems, five_groups):
    s = systems("trpcage")
    down = _binding(s, list(range(15, -1, -1)))
    up = _binding(s, list(range(16)))
    got_down, got_up = down.decompose(s.pos), up.decompose(s.pos)
    check(got_down, reference(s, range(16), "file", s.pos), what="descending list")
    assert np.abs(got_down[0] - got_up[0]).max() < SAME and abs(got_down[1] - got_up[1]) < SAME
    assert [int(down.member(m).scalar("last_evaluation_kind")) for m in range(3)] == [3, 3, 3]
    assert [int(down.member(m).scalar("group_members")) for m in range(3)] == [3, 3, 3]  # one launch set: 1 + 5 + 1 launches


# ---- 2. the device entry adds; NULL d_binding_energy --------------------------------------------------------------------------
def test_the_device_entry_adds_and_takes_no_u(gpu_required, systems, five_groups):
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    ligand = list(range(16))
    b = _binding(s, ligand)
    ref = reference(s, ligand, "jitter1", s.jittered(1))
    buf = Buffers(torch, s.n, fill=(1.0, 2.0))
    buf.load(s.jittered(1))
    pos0 = buf.pos.clone()
    buf.decompose(b)
    buf.decompose(b)
    buf.decompose(b, with_u=False)
    assert b.finish(buf.stream) == 0
    terms, u = buf.result()
    check((terms, 2.0 + 3.0 * ref[1]), ref, count=3, fill=(1.0, 2.0), what="three calls, planes")
    check((1.0 + 2.0 * ref[0], u), ref, count=2, fill=(1.0, 2.0), what="two calls with u")
    assert torch.equal(buf.pos, pos0)


# ---- 3. withheld: all or nothing, and the staging is cleared ------------------------------------------------------------------
@pytest.mark.parametrize("who", ["ligand", "receptor"])
def test_a_jump_of_one_atom_withholds_everything(gpu_required, systems, five_groups, who):
    """One heavy atom of the ligand (of the receptor) jumps 0.1 nm: that member and the complex are withheld, the third member
    is complete -- nothing reaches the caller's sentinel-filled buffers, bit for bit.  The repeat is right, and a following
    execute_device of the same binding is right: the complete member's planes and energy did not stay in the staging words (the
    members' energies of the force path are other words; what a stale staging buffer would spoil is the NEXT decomposition,
    checked last)."""
    torch = pytest.importorskip("torch")
    from tests.test_gpu_binding import Buffers as ForceBuffers
    from tests.test_gpu_binding import check as check_forces
    from tests.test_gpu_binding import reference as force_reference
    s = systems("trpcage")
    ligand = list(range(16))
    b = _binding(s, ligand)
    buf = Buffers(torch, s.n, fill=(SENTINEL, SENTINEL))
    buf.load(s.pos)
    buf.decompose(b)
    assert b.finish(buf.stream) == 0
    check(buf.result(), reference(s, ligand, "file", s.pos), fill=(SENTINEL, SENTINEL), what="before the jump")
    heavy = np.flatnonzero(s.ishydrogen == 0)
    atom = int(heavy[heavy < 16][2] if who == "ligand" else heavy[heavy >= 16][40])
    moved = _moved(s, atom)
    buf.load(moved)
    snap = buf.snapshot()
    buf.decompose(b)
    assert b.finish(buf.stream) == 1 and b.withheld() == [0]
    assert buf.unchanged_since(snap), "a withheld binding decomposition reached the caller's buffers"
    buf = Buffers(torch, s.n, fill=(SENTINEL, SENTINEL))
    buf.load(moved)
    buf.decompose(b)  # the repeat
    assert b.finish(buf.stream) == 0
    ref = reference(s, ligand, f"moved{atom}", moved)
    check(buf.result(), ref, fill=(SENTINEL, SENTINEL), what=f"the repeat after the {who}'s jump")
    fb = ForceBuffers(torch, s.n)
    fb.load(moved)
    fb.execute(b, 0.35)
    assert b.finish(fb.stream) == 0
    check_forces(fb.result(), force_reference(s, ligand, f"moved{atom}", moved), 0.35, what="execute_device behind it")
    fresh = Buffers(torch, s.n)
    fresh.load(moved)
    fresh.decompose(b)
    assert b.finish(fresh.stream) == 0
    check(fresh.result(), ref, what="the next decomposition")


def test_expect_jump_avoids_the_withholding(gpu_required, systems, five_groups):
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    ligand = list(range(16))
    b = _binding(s, ligand)
    buf = Buffers(torch, s.n)
    buf.load(s.pos)
    buf.decompose(b)
    assert b.finish(buf.stream) == 0
    moved = s.jittered(5) + np.array([0.1, 0.0, 0.0])
    buf = Buffers(torch, s.n)
    buf.load(moved)
    b.expect_jump()
    buf.decompose(b)
    assert b.finish(buf.stream) == 0
    check(buf.result(), reference(s, ligand, "jitter5_moved", moved), what="hinted jump")


# ---- 4. queues and interleaving ------------------------------------------------------------------------------------------------
def test_ten_decompositions_queued_on_one_stream(gpu_required, systems, five_groups):
    """One position buffer, ten calls, one finish: stream order protects the staging buffer -- ten times the terms."""
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    ligand = list(range(16))
    b = _binding(s, ligand)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        buf = Buffers(torch, s.n)
        buf.load(s.jittered(2))
        for _ in range(10):
            buf.decompose(b)
        assert b.finish(buf.stream) == 0
        check(buf.result(), reference(s, ligand, "jitter2", s.jittered(2)), count=10, what="ten queued")


def test_interleaved_with_the_other_binding_calls(gpu_required, systems, five_groups):
    torch = pytest.importorskip("torch")
    from tests.test_gpu_binding import Buffers as ForceBuffers
    from tests.test_gpu_binding import check as check_forces
    from tests.test_gpu_binding import reference as force_reference
    s = systems("trpcage")
    ligand = list(range(16))
    b = _binding(s, ligand)
    geoms = [s.jittered(k) for k in range(1, 7)]
    full = [ForceBuffers(torch, s.n) for _ in range(2)]
    eo = [ForceBuffers(torch, s.n) for _ in range(2)]
    dec = [Buffers(torch, s.n) for _ in range(2)]
    order = [(full[0], "F"), (dec[0], "D"), (eo[0], "E"), (dec[1], "D"), (full[1], "F"), (eo[1], "E")]
    for (x, what), g in zip(order, geoms):
        x.load(g)
    torch.cuda.synchronize()
    for x, what in order:
        if what == "F":
            x.execute(b, 0.35)
        elif what == "E":
            x.energy(b, 0.35)
        else:
            x.decompose(b)
    assert b.finish(dec[0].stream) == 0 and b.withheld() == []
    for k, ((x, what), g) in enumerate(zip(order, geoms), start=1):
        if what == "D":
            check(x.result(), reference(s, ligand, f"jitter{k}", g), what=f"call {k}")
        else:
            got = x.result()
            fref = force_reference(s, ligand, f"jitter{k}", g)
            if what == "E":
                assert not got[2].any()
                from tests.binding_restatement import combine
                got = (got[0], got[1], combine(*fref, 0.35)[2])
            check_forces(got, fref, 0.35, what=f"call {k} {what}")


# ---- 5. modes ------------------------------------------------------------------------------------------------------------------
def test_deterministic_mode_is_bit_identical(gpu_required, systems, five_groups):
    s = systems("trpcage")
    ligand = list(range(16))
    b = _binding(s, ligand, mode="deterministic")
    t1, u1 = b.decompose(s.pos)
    t2, u2 = b.decompose(s.pos)
    check((t1, u1), reference(s, ligand, "file", s.pos), what="deterministic")
    assert np.array_equal(t1, t2) and u1 == u2


def test_fast_mode_with_a_cutoff(gpu_required, systems, five_groups):
    s = systems("trpcage")
    ligand = list(range(16))
    b = _binding(s, ligand, mode="fast", cutoff=1.0)
    check(b.decompose(s.pos), reference(s, ligand, "file", s.pos, cutoff=1.0), what="fast, 1 nm")
    assert [int(b.member(m).scalar("group_members")) for m in range(3)] == [0, 0, 0]  # (every member ran alone)


# ---- 6. capture, host repeat, C++ ------------------------------------------------------------------------------------------------
def test_decompose_device_refuses_a_stream_capture(gpu_required, systems, five_groups):
    """Inside a capture the call is refused before the gather: nothing is launched, the capture ends cleanly and replays, no
    evaluation is logged, and the binding goes on."""
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    ligand = list(range(16))
    b = _binding(s, ligand)
    b.decompose(s.pos)
    buf = Buffers(torch, s.n)
    buf.load(s.jittered(1))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        buf.u.fill_(1.0)
        with pytest.raises(P.OpenMMException, match="captur"):
            b.decompose_device(buf.pos.data_ptr(), buf.terms.data_ptr(), buf.u.data_ptr(), torch.cuda.current_stream().cuda_stream)
    buf.u.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert buf.u.item() == 1.0 and not buf.terms.any().item()
    assert b.finish(buf.stream) == 0
    buf.u.zero_()
    buf.decompose(b)
    assert b.finish(buf.stream) == 0
    check(buf.result(), reference(s, ligand, "jitter1", s.jittered(1)), what="after the refusal")


def test_the_host_form_repeats_a_withheld_evaluation(gpu_required, systems, five_groups):
    s = systems("trpcage")
    ligand = list(range(16))
    b = _binding(s, ligand)
    check(b.decompose(s.pos), reference(s, ligand, "file", s.pos), what="host")
    moved = s.jittered(6) + np.array([0.0, 0.1, 0.0])  # every atom jumps: all three members are withheld once, repeated inside
    check(b.decompose(moved), reference(s, ligand, "jitter6_moved", moved), what="host across a jump")
    assert b.finish() == 0 and b.withheld() == []


def test_cxx_mirrors(gpu_required, systems, five_groups, tmp_path):
    """tests/cxx/TestHipBindingDecomposition.cpp through cpp/AGBNPForce.h."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(root, "openmm_agbnp_plugin_amd")
    exe = str(tmp_path / "TestHipBindingDecomposition")
    subprocess.run(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    os.path.join(root, "tests", "cxx", "TestHipBindingDecomposition.cpp"), "-o", exe, os.path.join(libdir, "libagbnp_hip.so"),
                    "-L/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    x = systems("trpcage")
    path = tmp_path / "trpcage.txt"
    r, g, a, q, h = x.params()
    np.savetxt(path, np.column_stack([r, g, a, q, np.asarray(h, dtype=float), x.pos]), fmt="%.17g")
    out = subprocess.run([exe, str(path), "16"], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
