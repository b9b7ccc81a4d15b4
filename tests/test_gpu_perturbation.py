"""GPU box: perturbation energies (include/agbnp_hip.h: agbnp_hip_set_parameter_sets, agbnp_hip_perturbed_energies_host /
_device) through the Python surface.  Every E_m against the CPU oracle created with set m
(tests/perturbation_restatement.py, oracle_energy: the reference; its formula is pinned on the CPU by
tests/test_perturbation_restatement.py) within TIGHT, scaled as energy_close scales it: on the protein fixtures, at every
compiled tier and off it, at the shapes where the launch can go wrong, with degenerate sets, in every mode, through the device
entry with its overflow log, and a context left exactly as a full evaluation leaves it.

The oracle energies of a (system, geometry, sets) are computed once and shared (REFERENCE)."""
import ctypes as C

import numpy as np
import pytest

import openmm_agbnp_plugin_amd as P
from openmm_agbnp_plugin_amd import _lib
from tests.edge_systems import edge_systems
from tests.gpu_helpers import SAME, TIGHT, energy_close
from tests.gpu_helpers import five  # noqa: F401
from tests.perturbation_restatement import ladder, oracle_energies, tables

pytestmark = pytest.mark.gpu

REFERENCE = {}


def own_set(s):
    return tuple(np.asarray(p, dtype=np.float64) for p in s.params()[1:4])


def three_sets(s):
    """The context's own parameters; charges x 0.9 with alpha x 1.1; gamma x 0.5."""
    g, a, q = own_set(s)
    return [(g, a, q), (g, 1.1 * a, 0.9 * q), (0.5 * g, a, q)]


def reference(s, tag, pos, sets, version=1, cutoff=None):
    key = (s.name, tag, len(sets), version, cutoff)
    if key not in REFERENCE:
        REFERENCE[key] = oracle_energies(s.params(), sets, pos, version=version, cutoff=cutoff)
        REFERENCE[key].setflags(write=False)
    return REFERENCE[key]


def _kernel(s, version=1, mode="reference", cutoff=None, sets=None):
    k = P.HipCalcAGBNPForceKernel(device=0, mode=mode)
    force = P.AGBNPForce.from_arrays(*s.params(), version=version)
    if cutoff is not None:
        force.setNonbondedMethod(P.AGBNPForce.CutoffNonPeriodic)
        force.setCutoffDistance(cutoff)
    k.initialize(force)
    if sets is not None:
        k.set_parameter_sets(*tables(sets))
    return k


def all_close(name, energies, ref, tol=TIGHT):
    assert energies.shape == ref.shape
    print(f"{name}: worst |E_m - reference| {float(np.abs(energies - ref).max()):.3e} over {len(ref)} sets")
    for e, eo in zip(energies, ref):
        energy_close(e, eo, tol)


def check(k, s, tag, pos, sets, version=1, cutoff=None):
    """One host call: every E_m against its oracle, the kind of the evaluation."""
    own, energies = k.perturbed_energies(pos)
    all_close(s.name, energies, reference(s, tag, pos, sets, version, cutoff))
    assert int(k.scalar("last_evaluation_kind")) == 5
    return own, energies


# ---- 1. parity -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["trpcage", "fixture264"])
def test_three_sets_on_the_protein_fixtures(gpu_required, systems, five, name):
    s = systems(name)
    sets = three_sets(s)
    k = _kernel(s, sets=sets)
    assert k.num_parameter_sets() == 3
    own, energies = check(k, s, "file", s.pos, sets)
    energy_close(energies[0], own)           # set 0 is the context's own parameters
    energy_close(k.energy(s.pos), own, SAME)  # ... and the returned energy is the energy-only evaluation's
    assert int(k.scalar("last_evaluation_kind")) != 5
    check(k, s, "jitter1", s.jittered(1), sets)  # another geometry on the same context


def test_two_sets_on_1dwc(gpu_required, systems, five):
    """Many tiles (2145)."""
    s = systems("1dwc")
    sets = three_sets(s)[:2]
    own, energies = check(_kernel(s, sets=sets), s, "file", s.pos, sets)
    energy_close(energies[0], own)


def test_the_context_stand_in(gpu_required, systems, five):
    s = systems("trpcage")
    sets = three_sets(s)
    ctx = P.AGBNPContext(P.AGBNPForce.from_arrays(*s.params(), version=1), device=0)
    ctx.setPositions(s.pos)
    own, energies = ctx.getPerturbedEnergies(*tables(sets))
    all_close("trpcage", energies, reference(s, "file", s.pos, sets))
    energy_close(own, ctx.getEnergy(), SAME)
    own, energies = ctx.getPerturbedEnergies(*tables(sets), groups=2)
    assert own == 0.0 and energies.shape == (3,) and not energies.any()


# ---- 2. tiers and padding ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 5, 16])
def test_every_tier_and_the_padded_sets(gpu_required, systems, five, count):
    """1: one set in the tier of 4, as a [N] array; 5: off-tier, three padded sets in the tier of 8; 16: the full table."""
    s = systems("trpcage")
    sets = ladder(s.params(), 16)[:count]
    k = _kernel(s)
    k.set_parameter_sets(*(tables(sets) if count > 1 else sets[0]))
    assert k.num_parameter_sets() == count
    own, energies = k.perturbed_energies(s.pos)
    all_close(f"trpcage M={count}", energies, reference(s, "ladder", s.pos, ladder(s.params(), 16))[:count])
    energy_close(energies[0], own)  # (rung 0 is the context's own)


def test_replaced_sets_of_another_size(gpu_required, systems, five):
    """16 sets, then 2: no stale table, no stale count; the generation and the launch counts do not move."""
    s = systems("trpcage")
    k = _kernel(s, sets=ladder(s.params(), 16))
    k.perturbed_energies(s.pos)
    state = (k.generation(), int(k.scalar("launches")), int(k.scalar("energy_only_launches")))
    sets = three_sets(s)[1:]
    k.set_parameter_sets(*tables(sets))
    assert k.num_parameter_sets() == 2
    assert (k.generation(), int(k.scalar("launches")), int(k.scalar("energy_only_launches"))) == state
    _, energies = k.perturbed_energies(s.pos)
    all_close("trpcage", energies, reference(s, "file", s.pos, three_sets(s))[1:])


# ---- 3. the shapes where the launch can go wrong -----------------------------------------------------------------------------------
EDGES = ("size_0_1", "size_1_33", "size_65_65", "size_129_257", "born_clamp", "born_clamp_strip_27")


@pytest.mark.parametrize("name", EDGES)
def test_block_edges_and_born_regimes(gpu_required, five, name):
    """No pair; one partial diagonal tile; a second block of one atom; an odd block count; capped Born radii; a block beyond the
    GB stage's far-strip bound (this launch has no far shortcut)."""
    s = edge_systems()[name]
    sets = three_sets(s)
    own, energies = check(_kernel(s, sets=sets), s, "file", s.pos, sets)
    energy_close(energies[0], own)


# ---- 4. degenerate sets --------------------------------------------------------------------------------------------------------
def test_degenerate_sets(gpu_required, systems, five):
    s = systems("trpcage")
    g, a, q = own_set(s)
    zero = np.zeros_like(q)
    one = zero.copy()
    one[17] = q[17] if q[17] != 0.0 else 0.5
    rng = np.random.default_rng(11)
    per_atom = np.where(s.ishydrogen != 0, 0.0, g * rng.uniform(0.5, 1.5, s.n))
    loud = np.where(s.ishydrogen != 0, 55.0, g)  # gammas on hydrogens count as 0
    sets = [(g, a, zero),       # cavity + vdW alone
            (zero, zero, q),    # GB alone
            (zero, zero, one),  # one charged atom: its self term, no pair term
            (per_atom, a, q),
            (zero, zero, zero)]
    k = _kernel(s, sets=sets + [(loud, a, q)])
    _, energies = k.perturbed_energies(s.pos)
    all_close("trpcage degenerate", energies[:5], reference(s, "degenerate", s.pos, sets))
    assert energies[4] == 0.0
    energy_close(energies[5], reference(s, "file", s.pos, three_sets(s))[0])


# ---- 5. versions and modes -------------------------------------------------------------------------------------------------------
def test_version_0_gives_the_cavity_term_only(gpu_required, systems, five):
    s = systems("fixture264")
    sets = three_sets(s)
    k = _kernel(s, version=0, sets=sets)
    own, energies = check(k, s, "file", s.pos, sets, version=0)
    assert abs(own - 872.5144) < 1e-3
    energy_close(energies[1], own)          # charges and alpha do not enter
    energy_close(energies[2], 0.5 * own)    # the cavity term is linear in gamma


def test_fast_mode_with_a_cutoff(gpu_required, systems, five):
    s = systems("trpcage")
    sets = three_sets(s)
    own, energies = check(_kernel(s, mode="fast", cutoff=1.0, sets=sets), s, "file", s.pos, sets, cutoff=1.0)
    energy_close(energies[0], own)
    assert abs(energies[0] - reference(s, "file", s.pos, sets)[0]) > 1e-3  # (the cutoff truncates)


def test_fast_single_gives_the_fp64_fast_modes_numbers(gpu_required, systems, five):
    s = systems("trpcage")
    sets = three_sets(s)
    k = _kernel(s, mode="fast+single", cutoff=1.0, sets=sets)
    before = k.energy(s.pos)
    check(k, s, "file", s.pos, sets, cutoff=1.0)
    assert abs(k.energy(s.pos) - before) < 1e-6  # (the context stays in its mode)


def test_deterministic_mode_is_bit_identical(gpu_required, systems, five):
    """Every workgroup's total is rounded to 2^-36 before its add: 11 + 2 totals per set on trpcage, under 1e-10 together."""
    s = systems("trpcage")
    sets = three_sets(s)
    k = _kernel(s, mode="deterministic", sets=sets)
    own1, e1 = check(k, s, "file", s.pos, sets)
    own2, e2 = k.perturbed_energies(s.pos)
    assert own1 == own2 and np.array_equal(e1, e2)


# ---- 6. the device entry and the contract ------------------------------------------------------------------------------------------
def test_the_device_entry_adds(gpu_required, systems, five):
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    sets = three_sets(s)
    k = _kernel(s, sets=sets)
    k.execute(s.pos, np.zeros((s.n, 3)))
    ref = reference(s, "jitter1", s.jittered(1), sets)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    pos = torch.tensor(s.jittered(1), dtype=torch.float64, device=dev).contiguous()
    pos0 = pos.clone()
    out = torch.full((3,), 1.0, dtype=torch.float64, device=dev)
    ene = torch.full((1,), 2.0, dtype=torch.float64, device=dev)
    lone = torch.zeros((3,), dtype=torch.float64, device=dev)
    k.perturbed_energies_device(pos.data_ptr(), out.data_ptr(), ene.data_ptr(), stream)
    k.perturbed_energies_device(pos.data_ptr(), out.data_ptr(), ene.data_ptr(), stream)
    k.perturbed_energies_device(pos.data_ptr(), lone.data_ptr(), None, stream)  # d_energy = NULL is accepted
    assert int(k.scalar("last_evaluation_kind")) == 5
    assert k.finish(stream) == 0, (k.withheld(), int(k.scalar("overflow_kinds")))
    torch.cuda.synchronize()
    all_close("twice", out.cpu().numpy(), 1.0 + 2.0 * ref, 2 * TIGHT)
    energy_close(ene.item(), 2.0 + 2.0 * ref[0], 2 * TIGHT)
    all_close("lone", lone.cpu().numpy(), ref)
    assert torch.equal(pos, pos0)


def test_a_jump_is_withheld_and_a_hint_prevents_it(gpu_required, systems, five):
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    sets = three_sets(s)
    k = _kernel(s, sets=sets)
    k.execute(s.pos, np.zeros((s.n, 3)))
    assert int(k.scalar("launches")) == 5
    heavy = np.flatnonzero(s.ishydrogen == 0)
    moved = s.pos.copy()
    moved[heavy[len(heavy) // 2], 0] += 0.06
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    pos = torch.tensor(moved, dtype=torch.float64, device=dev).contiguous()
    out = torch.full((3,), 1.0, dtype=torch.float64, device=dev)
    ene = torch.full((1,), 2.0, dtype=torch.float64, device=dev)
    k.perturbed_energies_device(pos.data_ptr(), out.data_ptr(), ene.data_ptr(), stream)
    assert k.finish(stream) == 1 and list(k.withheld()) == [0]
    torch.cuda.synchronize()
    assert (out == 1.0).all().item() and ene.item() == 2.0  # nothing was added to either output
    # the same call after the hint is complete (the masks of the withheld evaluation lie at `moved`: jump back first)
    k.execute(s.pos, np.zeros((s.n, 3)))
    k.expect_jump()
    k.perturbed_energies_device(pos.data_ptr(), out.data_ptr(), ene.data_ptr(), stream)
    assert k.finish(stream) == 0, (k.withheld(), int(k.scalar("overflow_kinds")))
    ref = reference(s, "moved", moved, sets)
    all_close("moved", out.cpu().numpy(), 1.0 + ref)
    energy_close(ene.item(), 2.0 + ref[0])
    assert int(k.scalar("launches")) == 5
    check(k, s, "file", s.pos, sets)  # the host entry point across a jump repeats by itself


def test_the_context_is_left_as_a_full_evaluation_leaves_it(gpu_required, systems, five):
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    sets = three_sets(s)
    k, twin = _kernel(s, sets=sets), _kernel(s)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    geoms = torch.tensor(np.stack([s.jittered(1), s.jittered(2)]), dtype=torch.float64, device=dev).contiguous()
    result = {}
    for who, kernel in (("with", k), ("without", twin)):
        kernel.execute(s.pos, np.zeros((s.n, 3)))
        state = (kernel.generation(), int(kernel.scalar("launches")), int(kernel.scalar("energy_only_launches")))
        assert state[1:] == (5, 4)
        frc = torch.zeros((s.n, 3), dtype=torch.float64, device=dev)
        ene = torch.zeros((1,), dtype=torch.float64, device=dev)
        if who == "with":
            out = torch.zeros((3,), dtype=torch.float64, device=dev)
            kernel.perturbed_energies_device(geoms[0].data_ptr(), out.data_ptr(), None, stream)
            assert int(kernel.scalar("last_evaluation_kind")) == 5
        else:
            spare = torch.zeros((1,), dtype=torch.float64, device=dev)
            kernel.energy_device(geoms[0].data_ptr(), spare.data_ptr(), stream)
        kernel.execute_device(geoms[1].data_ptr(), frc.data_ptr(), ene.data_ptr(), stream)
        assert int(kernel.scalar("last_evaluation_kind")) == 0
        assert kernel.finish(stream) == 0
        assert (kernel.generation(), int(kernel.scalar("launches")), int(kernel.scalar("energy_only_launches"))) == state
        result[who] = (ene.item(), frc.cpu().numpy())
    assert abs(result["with"][0] - result["without"][0]) < SAME and np.abs(result["with"][1] - result["without"][1]).max() < SAME
    all_close("jitter1", out.cpu().numpy(), reference(s, "jitter1", s.jittered(1), sets))


def test_update_parameters_keeps_the_sets_and_meets_them(gpu_required, systems, five):
    """copyParametersToContext() leaves the sets alone, and with set m as the context's own parameters energy() is E_m."""
    s = systems("trpcage")
    sets = three_sets(s)
    force = P.AGBNPForce.from_arrays(*s.params(), version=1)
    k = P.HipCalcAGBNPForceKernel(device=0)
    k.initialize(force)
    k.set_parameter_sets(*tables(sets))
    own0, e0 = k.perturbed_energies(s.pos)
    for m in (1, 2):
        g, a, q = sets[m]
        for i in range(s.n):
            force.setParticleParameters(i, s.radius[i], g[i], a[i], q[i], bool(s.ishydrogen[i]))
        k.copyParametersToContext(force)
        assert k.num_parameter_sets() == 3
        energy_close(k.energy(s.pos), e0[m])
        own, e = k.perturbed_energies(s.pos)
        energy_close(own, e0[m])
        assert np.abs(e - e0).max() < SAME  # the sets are independent of the context's own parameters
    all_close("trpcage", e0, reference(s, "file", s.pos, sets))


def test_refused_sets_keep_the_ones_before(gpu_required, systems, five):
    s = systems("trpcage")
    sets = three_sets(s)
    k = _kernel(s, sets=sets)
    lib = _lib.load()
    g, a, q = tables(sets)
    dp = lambda x: x.ctypes.data_as(C.POINTER(C.c_double))
    bad = _lib.ERR_INVALID_ARGUMENT
    assert lib.agbnp_hip_set_parameter_sets(k._h, s.n - 1, 3, dp(g), dp(a), dp(q)) == bad
    assert "particles" in _lib.last_error(k._h)
    assert lib.agbnp_hip_set_parameter_sets(k._h, s.n, 0, dp(g), dp(a), dp(q)) == bad
    assert lib.agbnp_hip_set_parameter_sets(k._h, s.n, 17, dp(g), dp(a), dp(q)) == bad
    assert lib.agbnp_hip_set_parameter_sets(k._h, s.n, 3, None, dp(a), dp(q)) == bad
    assert lib.agbnp_hip_set_parameter_sets(k._h, s.n, 3, dp(g), None, dp(q)) == bad
    assert lib.agbnp_hip_set_parameter_sets(k._h, s.n, 3, dp(g), dp(a), None) == bad
    assert lib.agbnp_hip_perturbed_energies_host(k._h, None, None, None) == bad
    assert lib.agbnp_hip_perturbed_energies_device(k._h, None, None, None, None) == bad
    with pytest.raises(P.OpenMMException):
        k.set_parameter_sets(g[:, :-1], a[:, :-1], q[:, :-1])
    assert k.num_parameter_sets() == 3
    check(k, s, "file", s.pos, sets)


def test_without_sets_the_calls_are_refused(gpu_required, systems, five):
    s = systems("trpcage")
    k = _kernel(s)
    assert k.num_parameter_sets() == 0
    with pytest.raises(P.OpenMMException, match="no parameter sets have been set"):
        k.perturbed_energies(s.pos)
    with pytest.raises(P.OpenMMException, match="no parameter sets have been set"):
        k.perturbed_energies_device(1, 2)
    f = np.zeros((s.n, 3))
    k.execute(s.pos, f)  # (the context goes on)
    assert f.any()


def test_the_device_entry_refuses_a_stream_capture(gpu_required, systems, five):
    """Inside a capture the call fails with INVALID_ARGUMENT, launches nothing, and the capture ends cleanly and replays."""
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    sets = three_sets(s)
    k = _kernel(s, sets=sets)
    k.execute(s.pos, np.zeros((s.n, 3)))
    dev = torch.device("cuda:0")
    pos = torch.tensor(s.jittered(1), dtype=torch.float64, device=dev).contiguous()
    out = torch.zeros((3,), dtype=torch.float64, device=dev)
    ene = torch.zeros((1,), dtype=torch.float64, device=dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ene.fill_(1.0)
        with pytest.raises(P.OpenMMException, match="captur"):
            k.perturbed_energies_device(pos.data_ptr(), out.data_ptr(), ene.data_ptr(), torch.cuda.current_stream().cuda_stream)
    ene.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert ene.item() == 1.0 and not out.any().item()
    assert int(k.scalar("launches")) == 5 and int(k.scalar("energy_only_launches")) == 4
    check(k, s, "jitter1", s.jittered(1), sets)
