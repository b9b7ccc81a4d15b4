"""GPU box: per-atom decomposition of an evaluation (include/agbnp_hip.h: agbnp_hip_decompose_host / _device).
Every one of the 4 N terms against the NumPy restatement built from the CPU oracle's vectors (tests/decomposition_restatement.py,
pinned on the CPU by tests/test_decomposition_restatement.py), at the sizes and in the modes where the new launch can go wrong, the
overflow log, and a context left exactly as a full evaluation leaves it.  The restatement of a geometry is computed once and
shared (REFS)."""
import numpy as np
import pytest

import openmm_agbnp_plugin_amd as P
from oracle import Oracle
from tests.decomposition_restatement import restate
from tests.edge_systems import edge_systems
from tests.gpu_helpers import SAME, TIGHT
from tests.gpu_helpers import close as _close
from tests.gpu_helpers import energy_close as _energy_close
from tests.gpu_helpers import five  # noqa: F401

pytestmark = pytest.mark.gpu

REFS = {}


def reference(s, tag, pos, version=1, cutoff=None, params=None):
    """(energy, terms[4, N]) of the restatement at `pos`, once per (system, tag, version, cutoff)."""
    key = (s.name, tag, version, cutoff)
    if key not in REFS:
        e, terms, _ = restate(params or s.params(), pos, version=version, cutoff=cutoff)
        terms.setflags(write=False)
        REFS[key] = (e, terms)
    return REFS[key]


def _kernel(s, version=1, mode="reference", cutoff=None):
    k = P.HipCalcAGBNPForceKernel(device=0, mode=mode)
    force = P.AGBNPForce.from_arrays(*s.params(), version=version)
    if cutoff is not None:
        force.setNonbondedMethod(P.AGBNPForce.CutoffNonPeriodic)
        force.setCutoffDistance(cutoff)
    k.initialize(force)
    return k


def terms_close(terms, ref, tol=TIGHT):
    assert terms.shape == ref.shape
    worst = np.abs(terms - ref).max(axis=1)
    print("worst |term - restatement| per plane:", worst)
    assert worst.max() < tol, f"terms differ by {worst} (planes cavity, vdw, gb_self, gb_pair)"


def check_host(k, s, tag, pos, version=1, cutoff=None):
    e_ref, ref = reference(s, tag, pos, version, cutoff)
    e, terms = k.decompose(pos)
    terms_close(terms, ref)
    _energy_close(e, e_ref)
    _energy_close(float(terms.sum()), e_ref)
    return e, terms


# ---- 1. parity, host entry -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["trpcage", "fixture264", "1dwc"])
def test_every_term_matches_the_restatement(gpu_required, systems, five, name):
    """(1dwc: the one case with many forests per workgroup.)"""
    s = systems(name)
    k = _kernel(s)
    e, terms = check_host(k, s, "file", s.pos)
    f = np.zeros((s.n, 3))
    _energy_close(e, k.execute(s.pos, f))
    assert int(k.scalar("last_evaluation_kind")) == 0
    if name == "trpcage":  # another geometry on the same context, and the Context stand-in
        check_host(k, s, "jitter1", s.jittered(1))
        ctx = P.AGBNPContext(P.AGBNPForce.from_arrays(*s.params(), version=1), device=0)
        ctx.setPositions(s.pos)
        e2, t2 = ctx.getEnergyDecomposition()
        terms_close(t2, reference(s, "file", s.pos)[1])
        assert abs(e2 - e) < SAME
        assert ctx.getEnergyDecomposition(groups=2)[0] == 0.0


def test_version_0_has_the_cavity_plane_only(gpu_required, systems, five):
    s = systems("fixture264")
    k = _kernel(s, version=0)
    e, terms = check_host(k, s, "file", s.pos, version=0)
    assert (terms[1:] == 0.0).all()
    assert abs(e - 872.5144) < 1e-3
    f = np.zeros((s.n, 3))
    _energy_close(e, k.execute(s.pos, f))


# ---- 2. edges --------------------------------------------------------------------------------------------------------
EDGES = ("size_0_1", "size_1_33", "size_65_65", "size_127_255", "size_129_257", "size_257_513", "born_clamp", "born_clamp_strip_27")


@pytest.mark.parametrize("name", EDGES)
def test_block_edges_and_capped_born_radii(gpu_required, five, name):
    """No heavy atom and no pair; one partial block (the diagonal tile only); a second block of one atom; last blocks of one atom
    and odd block counts; Born radii at the 2 nm cap; three blocks of which one lies beyond the GB stage's far-strip bound (the
    decomposition has no far shortcut: the far pairs are in plane 3)."""
    s = edge_systems()[name]
    k = _kernel(s)
    e, terms = check_host(k, s, "file", s.pos)
    if name == "size_0_1":
        assert terms[0, 0] == 0.0 and terms[3, 0] == 0.0
    if name == "born_clamp_strip_27":
        far = reference(s, "file", s.pos)[1][3][128:]
        assert np.abs(far).max() > 1e-3  # (block 2 has a pair energy worth resolving, most of it with its own atoms)


# ---- 3. modes --------------------------------------------------------------------------------------------------------
def test_fast_mode_with_a_cutoff(gpu_required, systems, five):
    s = systems("trpcage")
    k = _kernel(s, mode="fast", cutoff=1.0)
    check_host(k, s, "file", s.pos, cutoff=1.0)


def test_fast_mode_without_a_cutoff_is_the_reference_mode(gpu_required, systems, five):
    s = systems("trpcage")
    e_fast, t_fast = _kernel(s, mode="fast").decompose(s.pos)
    e_ref, t_ref = _kernel(s).decompose(s.pos)
    assert np.abs(t_fast - t_ref).max() < SAME and abs(e_fast - e_ref) < SAME
    terms_close(t_fast, reference(s, "file", s.pos)[1])


def test_fast_single_terms_are_those_of_the_fp64_fast_mode(gpu_required, systems, five):
    """The header's promise for fast+single: FP64 terms that sum to what the FP64 fast mode gives; the context stays in its mode."""
    s = systems("trpcage")
    k = _kernel(s, mode="fast+single", cutoff=1.0)
    before = k.energy(s.pos)
    check_host(k, s, "file", s.pos, cutoff=1.0)
    assert abs(k.energy(s.pos) - before) < 1e-6  # (as tests/test_gpu_energy_only.py compares two runs of that mode)
    assert abs(before - reference(s, "file", s.pos, cutoff=1.0)[0]) < 0.1


def test_deterministic_mode_is_bit_identical(gpu_required, systems, five):
    s = systems("trpcage")
    k = _kernel(s, mode="deterministic")
    e1, t1 = check_host(k, s, "file", s.pos)
    e2, t2 = k.decompose(s.pos)
    assert e1 == e2 and np.array_equal(t1, t2)


@pytest.mark.parametrize("flavour", ["rows0", "five0", "captured"])
def test_the_other_launch_sequences(gpu_required, systems, five, monkeypatch, flavour):
    """The tile kernels everywhere, the k_prep launch, and a context whose set the device names (captured and replayed once)."""
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    if flavour == "rows0":
        monkeypatch.setenv("AGBNP_HIP_ROWS", "0")
    if flavour == "five0":
        monkeypatch.setenv("AGBNP_HIP_FIVE_LAUNCHES", "0")
    k = _kernel(s)
    f0 = np.zeros((s.n, 3))
    k.execute(s.pos, f0)
    if flavour == "captured":
        dev = torch.device("cuda:0")
        cpos = torch.tensor(s.jittered(1), dtype=torch.float64, device=dev).contiguous()
        cfrc = torch.zeros((s.n, 3), dtype=torch.float64, device=dev)
        cene = torch.zeros((1,), dtype=torch.float64, device=dev)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            cfrc.zero_()
            cene.zero_()
            k.execute_device(cpos.data_ptr(), cfrc.data_ptr(), cene.data_ptr(), torch.cuda.current_stream().cuda_stream)
        g.replay()
        torch.cuda.synchronize()
        assert k.finish(torch.cuda.current_stream().cuda_stream) == 0
    launches = int(k.scalar("launches"))
    assert launches == (6 if flavour == "five0" else 5)
    check_host(k, s, "file", s.pos)
    check_host(k, s, "jitter1", s.jittered(1))
    assert int(k.scalar("launches")) == launches and int(k.scalar("energy_only_launches")) == 0


# ---- 4. device entry -------------------------------------------------------------------------------------------------
def test_the_device_entry_adds_and_writes_nothing_else(gpu_required, systems, five):
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    k = _kernel(s)
    f0 = np.zeros((s.n, 3))
    k.execute(s.pos, f0)
    e_ref, ref = reference(s, "jitter1", s.jittered(1))
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    pos = torch.tensor(s.jittered(1), dtype=torch.float64, device=dev).contiguous()
    pos0 = pos.clone()
    per_atom = torch.full((4, s.n), 1.0, dtype=torch.float64, device=dev)
    ene = torch.full((1,), 2.0, dtype=torch.float64, device=dev)
    lone = torch.zeros((4, s.n), dtype=torch.float64, device=dev)
    k.decompose_device(pos.data_ptr(), per_atom.data_ptr(), ene.data_ptr(), stream)
    k.decompose_device(pos.data_ptr(), per_atom.data_ptr(), ene.data_ptr(), stream)
    k.decompose_device(pos.data_ptr(), lone.data_ptr(), None, stream)  # d_energy = NULL is accepted
    assert int(k.scalar("last_evaluation_kind")) == 3
    assert k.finish(stream) == 0, (k.withheld(), int(k.scalar("overflow_kinds")))
    torch.cuda.synchronize()
    terms_close(per_atom.cpu().numpy(), 1.0 + 2.0 * ref, 2 * TIGHT)
    _energy_close(ene.item(), 2.0 + 2.0 * e_ref, 2 * TIGHT)
    terms_close(lone.cpu().numpy(), ref)
    assert torch.equal(pos, pos0)


# ---- 5. withheld -----------------------------------------------------------------------------------------------------
def test_a_jump_is_withheld_and_a_hint_prevents_it(gpu_required, systems, five):
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    k = _kernel(s)
    f0 = np.zeros((s.n, 3))
    k.execute(s.pos, f0)
    assert int(k.scalar("launches")) == 5
    heavy = np.flatnonzero(s.ishydrogen == 0)
    moved = s.pos.copy()
    moved[heavy[len(heavy) // 2], 0] += 0.06
    moved2 = moved.copy()
    moved2[heavy[len(heavy) // 3], 1] -= 0.06
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    pos = torch.tensor(np.stack([moved, moved2]), dtype=torch.float64, device=dev).contiguous()
    per_atom = torch.full((4, s.n), 1.0, dtype=torch.float64, device=dev)
    ene = torch.full((1,), 2.0, dtype=torch.float64, device=dev)
    k.decompose_device(pos[0].data_ptr(), per_atom.data_ptr(), ene.data_ptr(), stream)
    assert k.finish(stream) == 1 and list(k.withheld()) == [0]
    assert int(k.scalar("overflow_kinds")) & 16
    torch.cuda.synchronize()
    assert (per_atom == 1.0).all().item() and ene.item() == 2.0  # nothing was added to either output
    k.decompose_device(pos[0].data_ptr(), per_atom.data_ptr(), ene.data_ptr(), stream)  # the repeat
    assert k.finish(stream) == 0
    e_ref, ref = reference(s, "moved", moved)
    terms_close(per_atom.cpu().numpy(), 1.0 + ref)
    _energy_close(ene.item(), 2.0 + e_ref)
    # with the hint the next jump is not withheld
    per_atom.zero_()
    ene.zero_()
    k.expect_jump()
    k.decompose_device(pos[1].data_ptr(), per_atom.data_ptr(), ene.data_ptr(), stream)
    assert k.finish(stream) == 0, (k.withheld(), int(k.scalar("overflow_kinds")))
    e_ref2, ref2 = reference(s, "moved2", moved2)
    terms_close(per_atom.cpu().numpy(), ref2)
    _energy_close(ene.item(), e_ref2)
    assert int(k.scalar("launches")) == 5
    # the host entry point across a jump repeats by itself
    check_host(k, s, "file", s.pos)


# ---- 6. interleaving -------------------------------------------------------------------------------------------------
def test_interleaved_with_full_and_energy_only_evaluations(gpu_required, systems, five):
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    k = _kernel(s)
    oracle = Oracle(*s.params(), version=1)
    f0 = np.zeros((s.n, 3))
    k.execute(s.pos, f0)
    before = (int(k.scalar("launches")), int(k.scalar("energy_only_launches")), k.generation())
    assert before[:2] == (5, 4)
    geoms = [s.jittered(step) for step in (1, 2, 3, 4)]
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    pos = torch.tensor(np.stack(geoms), dtype=torch.float64, device=dev).contiguous()
    frc = torch.zeros((4, s.n, 3), dtype=torch.float64, device=dev)
    ene = torch.zeros((4,), dtype=torch.float64, device=dev)
    per_atom = torch.zeros((4, s.n), dtype=torch.float64, device=dev)
    k.execute_device(pos[0].data_ptr(), frc[0].data_ptr(), ene[0:1].data_ptr(), stream)
    k.decompose_device(pos[1].data_ptr(), per_atom.data_ptr(), ene[1:2].data_ptr(), stream)
    assert int(k.scalar("last_evaluation_kind")) == 3
    assert (int(k.scalar("launches")), int(k.scalar("energy_only_launches")), k.generation()) == before
    k.execute_device(pos[2].data_ptr(), frc[2].data_ptr(), ene[2:3].data_ptr(), stream)
    k.energy_device(pos[3].data_ptr(), ene[3:4].data_ptr(), stream)
    assert k.finish(stream) == 0, (k.withheld(), int(k.scalar("overflow_kinds")))
    assert (int(k.scalar("launches")), int(k.scalar("energy_only_launches")), k.generation()) == before
    e_got, f_got = ene.cpu().numpy(), frc.cpu().numpy()
    want = [oracle.execute(g) for g in geoms]
    _close(e_got[0], f_got[0], *want[0])
    _close(e_got[2], f_got[2], *want[2])
    _energy_close(e_got[1], want[1][0])
    _energy_close(e_got[3], want[3][0])
    assert not f_got[1].any() and not f_got[3].any()  # (no force buffer of the caller is written)
    terms_close(per_atom.cpu().numpy(), reference(s, "jitter2", geoms[1])[1])


# ---- 7. parameters ---------------------------------------------------------------------------------------------------
def test_halved_charges_quarter_the_pair_plane(gpu_required, systems, five):
    s = systems("trpcage")
    force = P.AGBNPForce.from_arrays(*s.params(), version=1)
    k = P.HipCalcAGBNPForceKernel(device=0)
    k.initialize(force)
    e0, t0 = k.decompose(s.pos)
    for i in range(s.n):
        r, g, a, q, h = force.getParticleParameters(i)
        force.setParticleParameters(i, r, g, a, 0.5 * q, h)
    k.copyParametersToContext(force)
    e1, t1 = k.decompose(s.pos)
    assert np.abs(t1[3] - 0.25 * t0[3]).max() < TIGHT
    assert np.abs(t1[2] - 0.25 * t0[2]).max() < TIGHT and np.abs(t1[:2] - t0[:2]).max() < TIGHT
    halved = (s.radius, s.gamma, s.alpha, 0.5 * s.charge, s.ishydrogen)
    e_ref, ref = reference(s, "halved", s.pos, params=halved)
    _energy_close(e1, e_ref)
    terms_close(t1, ref)


# ---- 8. capture ------------------------------------------------------------------------------------------------------
def test_decompose_device_refuses_a_stream_capture(gpu_required, systems, five):
    """Inside a capture the call fails with INVALID_ARGUMENT, launches nothing, and the capture ends cleanly and replays."""
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    k = _kernel(s)
    f0 = np.zeros((s.n, 3))
    k.execute(s.pos, f0)
    dev = torch.device("cuda:0")
    pos = torch.tensor(s.jittered(1), dtype=torch.float64, device=dev).contiguous()
    per_atom = torch.zeros((4, s.n), dtype=torch.float64, device=dev)
    ene = torch.zeros((1,), dtype=torch.float64, device=dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ene.fill_(1.0)
        with pytest.raises(P.OpenMMException, match="captur"):
            k.decompose_device(pos.data_ptr(), per_atom.data_ptr(), ene.data_ptr(), torch.cuda.current_stream().cuda_stream)
    ene.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert ene.item() == 1.0 and not per_atom.any().item()
    # the context goes on as before: still the five launches, still the restatement's terms
    assert int(k.scalar("launches")) == 5 and int(k.scalar("energy_only_launches")) == 4
    check_host(k, s, "jitter1", s.jittered(1))
