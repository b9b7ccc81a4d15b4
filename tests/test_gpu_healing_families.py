"""GPU box: forests HEALED inside the cavity launch (csrc/tree_bodies.h, cavity_forests, "(4) HEALING") on every entry family that
runs that body.  tests/test_gpu_healing.py and tests/test_gpu_openmm_entry.py pin healing through execute_device, execute_openmm
and a replayed graph; every family added since runs ANOTHER instantiation of the same body and had never met an overfull forest:

    energy_device                     k_tree_cavity_five + launch_energy_only_stages: no pseudo-volume launch -- the spare slots'
                                      topology is written and never replayed, the later sets' cavity energy must reach the slot's word
    decompose_ / pair_matrix_device   k_tree_cavity_five<.., SV1>: the enlarged-radius self volumes leave once per SET
    execute_ / energy_ / decompose_group   k_group_cavity_five<.., SV1>, k_group_pseudo: the workgroup number is relative to the
                                      member's own grid, the spare slots are numbered from the member's tree_blocks
    binding calls                     groups of three members of very different sizes between a gather and a combine launch
    deterministic mode                bit-identical whatever the packing: a healed evaluation is the most different packing there is

Two ways into the healing path, both at 264 to 272 atoms.  trpcage (272 atoms, 144 heavy) with a packing FROZEN from the host at
eight whole subtrees per forest (tests/gpu_helpers.py, freeze_packing): 18 forests of about 720 nodes in stores of 432, rebuilt in
halves, the later sets in spare work slots.  fixture264 (264 atoms, 136 heavy) on a FRESH context: its first evaluation runs one
subtree per work slot and meets a lone subtree beyond the store -- the four parts of a four-way share, no hook.

The protocol is that of test_overfull_forests_are_healed_inside_the_tree_launch: settle every context with two evaluations and
finish(); freeze; zero the outputs; queue the evaluations under test with no finish() in between; finish().  Always: nothing is
withheld, no capacity variant is raised, the generation stays, healed_forests > 0 on every frozen context and == 0 on every healthy
one.  Healing is a function of the geometry and the packing alone, so a frozen context's healed_forests is that of a second frozen
context run through execute_device -- the path the two files above pin -- over the same geometries (HEALED; never a literal count).

References and tolerances are the project's own: Oracle.execute, tests/decomposition_restatement.py,
tests/pair_matrix_restatement.py, tests/binding_restatement.py, tests/binding_decomposition_restatement.py; TIGHT = 1e-7 against a
reference (energies on energy_close's scale, sums of c evaluations c times), SAME = 1e-9 against a twin context of the same system
that is not frozen and runs the same call alone.  A reference of a geometry is computed once and shared."""
import os

import numpy as np
import pytest

import openmm_agbnp_plugin_amd as P
from oracle import Oracle
from tests.binding_restatement import combine
from tests.decomposition_restatement import restate
from tests.gpu_helpers import SAME, TIGHT, energy_close, freeze_packing, kernel_of
from tests.gpu_helpers import five_groups  # noqa: F401
from tests.pair_matrix_restatement import restate_matrix
from tests.test_gpu_binding import reference as binding_reference
from tests.test_gpu_binding_decomposition import reference as binding_decomposition_reference

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STORE = 432  # nodes of the smallest store (capacity variant 0)
SENTINEL = -1234.5678
LIGAND = list(range(16))  # of trpcage, as tests/test_gpu_binding.py has it
FOUR_PART_SEEDS = (2, 3, 5, 10)  # fixture264.jittered(seed): a lone subtree beyond the store on a fresh context
ORACLES, WANT, TERMS, HEALED = {}, {}, {}, {}
WORST = {}  # family -> [worst deviation against the reference, against the twin] (printed by every comparison)


# ---- references, computed once -------------------------------------------------------------------------------------------------
def want(s, version, seed):
    """(energy, forces) of the oracle at s.jittered(seed)."""
    key = (s.name, version, seed)
    if key not in WANT:
        if key[:2] not in ORACLES:
            ORACLES[key[:2]] = Oracle(*s.params(), version=version)
        e, f = ORACLES[key[:2]].execute(s.jittered(seed))
        f.setflags(write=False)
        WANT[key] = (e, f)
    return WANT[key]


def want_terms(s, version, seed):
    """(energy, terms[4, N]) of the decomposition's restatement at s.jittered(seed)."""
    key = (s.name, version, seed)
    if key not in TERMS:
        e, terms, _ = restate(s.params(), s.jittered(seed), version=version)
        terms.setflags(write=False)
        TERMS[key] = (e, terms)
    return TERMS[key]


def note(family, what, ref=0.0, twin=0.0):
    w = WORST.setdefault(family, [0.0, 0.0])
    w[0], w[1] = max(w[0], float(ref)), max(w[1], float(twin))
    print(f"[{family}] {what}: against the reference {ref:.3e}, against the twin {twin:.3e}  (family so far {w[0]:.3e} / {w[1]:.3e})")


# ---- contexts ------------------------------------------------------------------------------------------------------------------
def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


class Out:
    """Device buffers of one evaluation of one context: positions, forces, energy, planes (torch tensors)."""

    def __init__(self, torch, s, seed, fill=0.0):
        dev = torch.device("cuda:0")
        self.s, self.seed = s, seed
        self.pos = torch.tensor(s.jittered(seed), dtype=torch.float64, device=dev).contiguous()
        self.frc = torch.full((s.n, 3), fill, dtype=torch.float64, device=dev)
        self.ene = torch.zeros((1,), dtype=torch.float64, device=dev)
        self.terms = torch.zeros((4, s.n), dtype=torch.float64, device=dev)

    def single(self, kind, k, stream):
        if kind == "F":
            k.execute_device(self.pos.data_ptr(), self.frc.data_ptr(), self.ene.data_ptr(), stream)
        elif kind == "E":
            k.energy_device(self.pos.data_ptr(), self.ene.data_ptr(), stream)
        else:
            k.decompose_device(self.pos.data_ptr(), self.terms.data_ptr(), self.ene.data_ptr(), stream)

    def result(self):
        return self.ene.item(), self.frc.cpu().numpy(), self.terms.cpu().numpy()


def group_call(kind, ks, outs, stream):
    pos, ene = [o.pos.data_ptr() for o in outs], [o.ene.data_ptr() for o in outs]
    if kind == "F":
        P.execute_group(ks, pos, [o.frc.data_ptr() for o in outs], ene, stream)
    elif kind == "E":
        P.energy_group(ks, pos, ene, stream)
    else:
        P.decompose_group(ks, pos, [o.terms.data_ptr() for o in outs], ene, stream)


def settle(torch, k, s, seeds):
    """Two evaluations on the engine's own packing, read with finish()."""
    stream = _stream(torch)
    outs = [Out(torch, s, seed) for seed in seeds]
    torch.cuda.synchronize()
    for o in outs:
        o.single("F", k, stream)
    assert k.finish(stream) == 0, (list(k.withheld()), int(k.scalar("overflow_kinds")))
    assert int(k.scalar("variant")) == 0


def healed_through_execute_device(torch, s, version, seeds, settle_seeds, mode="reference"):
    """healed_forests of a second frozen context of the same system run through execute_device over the same geometries."""
    key = (s.name, version, tuple(seeds), tuple(settle_seeds), mode)
    if key not in HEALED:
        stream = _stream(torch)
        k = kernel_of(s.params(), version, mode)
        settle(torch, k, s, settle_seeds)
        freeze_packing(k, s.nheavy)
        outs = [Out(torch, s, seed) for seed in seeds]
        torch.cuda.synchronize()
        for o in outs:
            o.single("F", k, stream)
        assert k.finish(stream) == 0, (list(k.withheld()), int(k.scalar("overflow_kinds")))
        HEALED[key] = int(k.scalar("healed_forests"))  # (its numbers are the business of tests/test_gpu_healing.py)
        print(f"healed_forests of a frozen {s.name} (version {version}, {mode}) through execute_device over {tuple(seeds)}: {HEALED[key]}")
        assert HEALED[key] > 0
    return HEALED[key]


def state(k):
    return k.generation(), int(k.scalar("variant"))


def check_member(family, kind, out, version, twin_out=None, count=1):
    """One member's outputs of one evaluation of `kind` against the reference (TIGHT) and its lone twin's (SAME)."""
    s, seed = out.s, out.seed
    e, f, terms = out.result()
    eo, fo = want(s, version, seed)
    te, tf, tt = twin_out.result() if twin_out is not None else (e, f, terms)
    what = f"{s.name} jittered({seed}) {kind}"
    note(family, what + " energy", abs(e - eo), abs(e - te))
    energy_close(e, eo)
    energy_close(e, te, tol=SAME)
    if kind == "F":
        note(family, what + " forces", np.abs(f - fo).max(), np.abs(f - tf).max())
        assert np.abs(f - fo).max() < TIGHT, f"forces differ by {np.abs(f - fo).max():.3e}"
        assert np.abs(f - tf).max() < SAME
    else:
        assert (f == SENTINEL).all(), "a force buffer was written"
    if kind == "D":
        e_ref, ref = want_terms(s, version, seed)
        worst = np.abs(terms - ref).max(axis=1)
        note(family, what + f" planes {worst}", worst.max(), np.abs(terms - tt).max())
        assert worst.max() < TIGHT, f"terms differ by {worst} (planes cavity, vdw, gb_self, gb_pair)"
        assert np.abs(terms - tt).max() < SAME
        energy_close(e, e_ref)
        energy_close(float(terms.sum()), eo)
        if version == 0:
            assert (terms[1:] == 0.0).all()
    else:
        assert not terms.any()


# ---- 1. energy-only, one context -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("version", [1, 0])
def test_energy_only_evaluations_heal_and_leave_no_stale_spare_slot(gpu_required, systems, five_groups, version):
    """k_tree_cavity_five followed by launch_energy_only_stages: there is no pseudo-volume launch, so the spare slots' topology is
    written and never replayed, and the cavity energy of the later sets must have reached epart[2 slot] by itself.  energy_device,
    execute_device, energy_device, execute_device on four geometries, queued: every energy word is the oracle's, the one force
    buffer holds the oracle's sum over the two full evaluations (a full evaluation behind an energy-only one replays ITS spare
    slots, not the ones left there), the fast path ran (kind 1, scalar 18)."""
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    stream = _stream(torch)
    k = kernel_of(s.params(), version)
    settle(torch, k, s, (0, 1))
    assert int(k.scalar("energy_only_launches")) == (4 if version == 1 else 2)
    freeze_packing(k, s.nheavy)
    seeds = (2, 3, 4, 5)
    outs = [Out(torch, s, seed) for seed in seeds]
    frc = outs[1].frc
    torch.cuda.synchronize()
    gen = state(k)
    kinds = []
    for i, o in enumerate(outs):
        if i % 2 == 0:
            k.energy_device(o.pos.data_ptr(), o.ene.data_ptr(), stream)
        else:
            k.execute_device(o.pos.data_ptr(), frc.data_ptr(), o.ene.data_ptr(), stream)
        kinds.append(int(k.scalar("last_evaluation_kind")))
    assert k.finish(stream) == 0, (list(k.withheld()), int(k.scalar("overflow_kinds")))
    assert kinds == [1, 0, 1, 0]
    assert int(k.scalar("energy_only_launches")) == (4 if version == 1 else 2)
    assert state(k) == gen
    healed = int(k.scalar("healed_forests"))
    assert healed == healed_through_execute_device(torch, s, version, seeds, (0, 1))
    family = f"energy-only v{version}"
    for o in outs:
        e, eo = o.ene.item(), want(s, version, o.seed)[0]
        note(family, f"jittered({o.seed}) energy", abs(e - eo))
        energy_close(e, eo)
    f_want = want(s, version, seeds[1])[1] + want(s, version, seeds[3])[1]
    df = np.abs(frc.cpu().numpy() - f_want).max()
    note(family, "force sum of the two full evaluations", df)
    assert df < 2 * TIGHT
    assert not outs[0].frc.any().item() and not outs[2].frc.any().item()


# ---- 2. decomposition, one context ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("version", [1, 0])
def test_a_decomposition_heals(gpu_required, systems, five_groups, version):
    """k_tree_cavity_five<.., SV1>: the enlarged-radius self volumes are added once per set (S.at[9] zeroed again between sets, a
    root's own sphere once per subtree).  Three geometries queued on a frozen context and on a healthy twin: all 4 N terms are the
    restatement's and the twin's, the total is the oracle's."""
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    stream = _stream(torch)
    k, twin = kernel_of(s.params(), version), kernel_of(s.params(), version)
    for x in (k, twin):
        settle(torch, x, s, (0, 1))
    freeze_packing(k, s.nheavy)
    seeds = (2, 3, 4)
    outs = [Out(torch, s, seed, SENTINEL) for seed in seeds]
    touts = [Out(torch, s, seed, SENTINEL) for seed in seeds]
    torch.cuda.synchronize()
    gen = state(k)
    for o, t in zip(outs, touts):
        o.single("D", k, stream)
        t.single("D", twin, stream)
    assert int(k.scalar("last_evaluation_kind")) == 3
    assert k.finish(stream) == 0, (list(k.withheld()), int(k.scalar("overflow_kinds")))
    assert twin.finish(stream) == 0
    assert state(k) == gen
    assert int(k.scalar("healed_forests")) == healed_through_execute_device(torch, s, version, seeds, (0, 1))
    assert int(twin.scalar("healed_forests")) == 0
    for o, t in zip(outs, touts):
        check_member(f"decomposition v{version}", "D", o, version, t)


def test_the_enlarged_radius_self_volumes_of_a_healed_evaluation(gpu_required, systems, five_groups):
    """With the diagnostics on, a full evaluation collects the enlarged-radius self volumes through the same SV1 branches: on a
    frozen context they are the oracle's selfvol_large to 1e-12 relative, and selfvol_vdw with them."""
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    stream = _stream(torch)
    k = kernel_of(s.params())
    k.set_diagnostics(True)  # (before the freeze: the switch derives the argument blocks anew, which ends a freeze)
    settle(torch, k, s, (0, 1))
    freeze_packing(k, s.nheavy)
    out = Out(torch, s, 2)
    torch.cuda.synchronize()
    out.single("F", k, stream)
    assert k.finish(stream) == 0, (list(k.withheld()), int(k.scalar("overflow_kinds")))
    assert int(k.scalar("healed_forests")) == healed_through_execute_device(torch, s, 1, (2,), (0, 1))
    oracle = Oracle(*s.params(), version=1)
    oracle.execute(s.jittered(2))
    for name in ("selfvol_large", "selfvol_vdw"):
        got, ref = k.vector(name), oracle.vector(name)
        assert ref[s.ishydrogen == 0].min() > 0.0
        rel = np.abs(got - ref)[ref != 0.0] / np.abs(ref[ref != 0.0])
        note("self volumes (diagnostics)", f"{name}: worst relative deviation", rel.max())
        assert rel.max() < 1e-12 and (got[ref == 0.0] == 0.0).all()
    check_member("self volumes (diagnostics)", "F", out, 1)


# ---- 3. pair matrix, one context -----------------------------------------------------------------------------------------------
def test_a_pair_matrix_heals(gpu_required, systems, five_groups):
    """pair_matrix_device runs the SV1 cavity instantiation too: the 20 x 20 residue matrix of a frozen trpcage is the restatement's
    cell by cell; its rows sum to the residues' shares of the decomposition's terms and all of it to the energy."""
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    stream = _stream(torch)
    sets, labels = P.load_sets(os.path.join(GOLDEN, "residues_trpcage.txt"))
    S = len(labels)
    k, twin = kernel_of(s.params()), kernel_of(s.params())
    for x in (k, twin):
        x.set_atom_sets(sets)
        settle(torch, x, s, (0, 1))
    freeze_packing(k, s.nheavy)
    dev = torch.device("cuda:0")
    out = Out(torch, s, 2)
    matrix, tmatrix = (torch.zeros((S, S), dtype=torch.float64, device=dev) for _ in range(2))
    tene = torch.zeros((1,), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    gen = state(k)
    k.pair_matrix_device(out.pos.data_ptr(), matrix.data_ptr(), out.ene.data_ptr(), stream)
    twin.pair_matrix_device(out.pos.data_ptr(), tmatrix.data_ptr(), tene.data_ptr(), stream)
    assert int(k.scalar("last_evaluation_kind")) == 4
    assert k.finish(stream) == 0, (list(k.withheld()), int(k.scalar("overflow_kinds")))
    assert twin.finish(stream) == 0
    assert state(k) == gen
    assert int(k.scalar("healed_forests")) == healed_through_execute_device(torch, s, 1, (2,), (0, 1))
    assert int(twin.scalar("healed_forests")) == 0
    e_ref, ref, _ = restate_matrix(s.params(), s.jittered(2), sets, S)
    m, tm, e = matrix.cpu().numpy(), tmatrix.cpu().numpy(), out.ene.item()
    note("pair matrix", "cells", np.abs(m - ref).max(), np.abs(m - tm).max())
    assert np.abs(m - ref).max() < TIGHT
    assert np.abs(m - tm).max() < SAME
    assert np.abs(m - m.T).max() < SAME
    energy_close(e, e_ref)
    energy_close(e, want(s, 1, 2)[0])
    energy_close(e, tene.item(), tol=SAME)
    energy_close(float(m.sum()), e)
    shares = np.zeros(S)
    np.add.at(shares, np.asarray(sets), want_terms(s, 1, 2)[1].sum(axis=0))
    note("pair matrix", "row sums against the decomposition's shares", np.abs(m.sum(axis=1) - shares).max())
    assert np.abs(m.sum(axis=1) - shares).max() < TIGHT


# ---- 4. the four-part path through the families --------------------------------------------------------------------------------
def fresh_twin(torch, s, seed):
    """execute_device on a fresh context at jittered(seed): (healed_forests, max_subtree_nodes) -- what decides whether the seed
    meets a lone subtree beyond the store on the device."""
    key = ("fresh", s.name, seed)
    if key not in HEALED:
        k = kernel_of(s.params())
        out = Out(torch, s, seed)
        torch.cuda.synchronize()
        out.single("F", k, _stream(torch))
        assert k.finish(_stream(torch)) == 0, (list(k.withheld()), int(k.scalar("overflow_kinds")))
        HEALED[key] = (int(k.scalar("healed_forests")), int(k.scalar("max_subtree_nodes")))
        print(f"fresh {s.name} at jittered({seed}) through execute_device: healed_forests, max_subtree_nodes = {HEALED[key]}")
    return HEALED[key]


def four_part_checks(torch, s, k, seed):
    assert int(k.scalar("variant")) == 0 and int(k.scalar("pack_level")) == 0
    assert int(k.scalar("healed_forests")) >= 1
    assert int(k.scalar("max_subtree_nodes")) > STORE
    assert (int(k.scalar("healed_forests")), int(k.scalar("max_subtree_nodes"))) == fresh_twin(torch, s, seed)


@pytest.mark.parametrize("kind", ["E", "D"])
def test_a_lone_subtree_in_four_parts_through_a_single_call(gpu_required, systems, five_groups, kind):
    """fixture264 at jittered(2), (3), (5), (10) -- seeds used: all four; the device counts 447, 445, 447 and 449 nodes in the
    largest subtree (the CPU oracle, without the root atom, 446, 444, 446, 448), decided by execute_device on a fresh twin
    (fresh_twin) -- each on a FRESH context whose first evaluation is the call under test (energy_device, decompose_device): one
    subtree per work slot, a lone subtree beyond the 432-node store built as the four parts of a four-way share, the later ones in
    spare slots (healed_forests = 2 at every seed).  Nothing is withheld; the numbers are the reference's."""
    torch = pytest.importorskip("torch")
    s = systems("fixture264")
    stream = _stream(torch)
    for seed in FOUR_PART_SEEDS:
        k = kernel_of(s.params())
        out = Out(torch, s, seed, SENTINEL)
        torch.cuda.synchronize()
        out.single(kind, k, stream)
        assert k.finish(stream) == 0, (seed, list(k.withheld()), int(k.scalar("overflow_kinds")))
        four_part_checks(torch, s, k, seed)
        check_member(f"four parts, {dict(E='energy_device', D='decompose_device')[kind]}", kind, out, 1)


@pytest.mark.parametrize("kind", ["E", "D"])
def test_a_lone_subtree_in_four_parts_through_a_group(gpu_required, systems, five_groups, kind):
    """Three fresh fixture264 contexts at jittered(2), (3), (5) in one energy_group (decompose_group) call, their first
    evaluation: every member meets its lone subtree beyond the store inside the shared launch and builds it in four parts."""
    torch = pytest.importorskip("torch")
    s = systems("fixture264")
    stream = _stream(torch)
    seeds = FOUR_PART_SEEDS[:3]
    ks = [kernel_of(s.params()) for _ in seeds]
    outs = [Out(torch, s, seed, SENTINEL) for seed in seeds]
    torch.cuda.synchronize()
    group_call(kind, ks, outs, stream)
    assert [k.finish(stream) for k in ks] == [0] * 3, [(list(k.withheld()), int(k.scalar("overflow_kinds"))) for k in ks]
    assert [int(k.scalar("group_members")) for k in ks] == [3] * 3
    for k, o in zip(ks, outs):
        four_part_checks(torch, s, k, o.seed)
        check_member(f"four parts, {dict(E='energy_group', D='decompose_group')[kind]}", kind, o, 1)


# ---- 5. groups with healing members --------------------------------------------------------------------------------------------
def group_with_frozen_members(torch, systems, kind, version, frozen, order):
    """A group of trpcage at three jitters and fixture264 (`order`: the members' systems, "T" or "F"), all settled, the members
    in `frozen` frozen; one call of `kind`, and every member's lone twin (not frozen) through the single call of the same kind."""
    stream = _stream(torch)
    members = [systems("trpcage" if x == "T" else "fixture264") for x in order]
    base = [100 * m for m in range(len(members))]
    ks = [kernel_of(s.params(), version) for s in members]
    twins = [kernel_of(s.params(), version) for s in members]
    for k, t, s, b in zip(ks, twins, members, base):
        settle(torch, k, s, (b, b + 1))
        settle(torch, t, s, (b, b + 1))
    for m in frozen:
        assert order[m] == "T"
        freeze_packing(ks[m], members[m].nheavy)
    outs = [Out(torch, s, b + 2, 0.0 if kind == "F" else SENTINEL) for s, b in zip(members, base)]
    touts = [Out(torch, s, b + 2, 0.0 if kind == "F" else SENTINEL) for s, b in zip(members, base)]
    torch.cuda.synchronize()
    gens = [state(k) for k in ks]
    group_call(kind, ks, outs, stream)
    for t, o in zip(twins, touts):
        o.single(kind, t, stream)
    assert [k.finish(stream) for k in ks] == [0] * len(ks), [(list(k.withheld()), int(k.scalar("overflow_kinds"))) for k in ks]
    assert [t.finish(stream) for t in twins] == [0] * len(ks)
    assert [int(k.scalar("group_members")) for k in ks] == [len(ks)] * len(ks)  # (every member really shares)
    assert [int(k.scalar("last_evaluation_kind")) for k in ks] == [dict(F=0, E=1, D=3)[kind]] * len(ks)
    assert [state(k) for k in ks] == gens
    family = f"{dict(F='execute_group', E='energy_group', D='decompose_group')[kind]} v{version}"
    for m, (k, t, s, b, o, to) in enumerate(zip(ks, twins, members, base, outs, touts)):
        healed = int(k.scalar("healed_forests"))
        if m in frozen:
            assert healed == healed_through_execute_device(torch, s, version, (b + 2,), (b, b + 1)), f"member {m}"
        else:
            assert healed == 0, f"healthy member {m} healed {healed} forests"
        assert int(t.scalar("healed_forests")) == 0
        check_member(family, kind, o, version, to)


POSITIONS = {"first": ((0,), "TTTF"), "middle": ((1,), "TTTF"), "last": ((3,), "TTFT"), "all": ((0, 1, 3), "TTFT")}


@pytest.mark.parametrize("kind", ["F", "E", "D"])
@pytest.mark.parametrize("position,version", [("first", 1), ("middle", 1), ("last", 1), ("all", 1), ("middle", 0)])
def test_a_group_with_healing_members(gpu_required, systems, five_groups, kind, position, version):
    """k_group_cavity_five<.., SV1>, k_group_pseudo, k_group_energy_roles, k_group_outputs[_energy]: the healing member's
    workgroup number is relative to its own grid, its spare slots are numbered from ITS tree_blocks, and k_group_pseudo must find
    them at the number it recomputes from the member's forest_blocks and pseudo_blocks -- beside members that do not heal.
    trpcage at three jitters and fixture264 in one launch set; exactly one trpcage member frozen, first, in the middle or last in
    the group (version 0: in the middle), or all three of them: execute_group, energy_group, decompose_group."""
    torch = pytest.importorskip("torch")
    frozen, order = POSITIONS[position]
    group_with_frozen_members(torch, systems, kind, version, frozen, order)


# ---- 6. mixed kinds on the same members ----------------------------------------------------------------------------------------
def test_mixed_group_kinds_on_a_group_with_a_healing_member(gpu_required, systems, five_groups):
    """execute_group, energy_group, decompose_group, execute_group on the same four members -- the second one frozen -- with fixed
    position buffers (the geometries are copied in on the calls' stream) and no finish() in between, twice over: every output is
    the reference's, and after the first call of each parity no argument block is rewritten (include/agbnp_hip.h: scalar 21 stands
    still in a steady run of group calls with fixed position buffers) -- a frozen member does not break that."""
    torch = pytest.importorskip("torch")
    members = [systems("trpcage"), systems("trpcage"), systems("trpcage"), systems("fixture264")]
    base = [100 * m for m in range(4)]
    ks = [kernel_of(s.params()) for s in members]
    for k, s, b in zip(ks, members, base):
        settle(torch, k, s, (b, b + 1))
    freeze_packing(ks[1], members[1].nheavy)
    calls = "FEDF" * 2
    dev = torch.device("cuda:0")
    outs = [[Out(torch, s, b + 2 + c, 0.0 if kind == "F" else SENTINEL) for s, b in zip(members, base)] for c, kind in enumerate(calls)]
    pos = [torch.zeros((s.n, 3), dtype=torch.float64, device=dev) for s in members]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    assert side.cuda_stream != 0
    gens = [state(k) for k in ks]
    writes = []
    with torch.cuda.stream(side):
        for kind, row in zip(calls, outs):
            for p, o in zip(pos, row):
                p.copy_(o.pos)
                o.pos = p  # (the fixed buffer: the geometry is in it when the call's launches run, on this stream)
            group_call(kind, ks, row, side.cuda_stream)
            assert [int(k.scalar("last_evaluation_kind")) for k in ks] == [dict(F=0, E=1, D=3)[kind]] * 4
            writes.append([int(k.scalar("group_block_writes")) for k in ks])
    assert [k.finish(side.cuda_stream) for k in ks] == [0] * 4, [(list(k.withheld()), int(k.scalar("overflow_kinds"))) for k in ks]
    torch.cuda.synchronize()
    print("group_block_writes after each call:", writes)
    assert all(w == writes[1] for w in writes[2:]), "a steady run of mixed group calls rewrote an argument block"
    assert [int(k.scalar("group_block_writes")) for k in ks] == writes[1]
    assert [int(k.scalar("group_members")) for k in ks] == [4] * 4
    assert [state(k) for k in ks] == gens
    seeds = tuple(base[1] + 2 + c for c in range(len(calls)))
    assert int(ks[1].scalar("healed_forests")) == healed_through_execute_device(torch, members[1], 1, seeds, (base[1], base[1] + 1))
    assert [int(ks[m].scalar("healed_forests")) for m in (0, 2, 3)] == [0, 0, 0]
    for c, (kind, row) in enumerate(zip(calls, outs)):
        for o in row:
            check_member(f"mixed group kinds, call {c} ({kind})", kind, o, 1)


# ---- 7. binding ----------------------------------------------------------------------------------------------------------------
class BindingOut:
    """The caller's device buffers of one binding evaluation."""

    def __init__(self, torch, s, seed, fill=0.0):
        dev = torch.device("cuda:0")
        self.s, self.seed = s, seed
        self.pos = torch.tensor(s.jittered(seed), dtype=torch.float64, device=dev).contiguous()
        self.frc = torch.full((s.n, 3), fill, dtype=torch.float64, device=dev)
        self.ene, self.u = (torch.zeros((1,), dtype=torch.float64, device=dev) for _ in range(2))
        self.terms = torch.zeros((4, s.n), dtype=torch.float64, device=dev)

    def call(self, kind, b, lam, stream):
        if kind == "F":
            b.execute_device(self.pos.data_ptr(), lam, self.frc.data_ptr(), self.ene.data_ptr(), self.u.data_ptr(), stream)
        elif kind == "E":
            b.energy_device(self.pos.data_ptr(), lam, self.ene.data_ptr(), self.u.data_ptr(), stream)
        else:
            b.decompose_device(self.pos.data_ptr(), self.terms.data_ptr(), self.u.data_ptr(), stream)

    def check(self, family, kind, lam):
        """E_lam, u and F_lam against tests/binding_restatement.py, D[t][i] against tests/binding_decomposition_restatement.py."""
        s, tag = self.s, f"jitter{self.seed}"
        pos = s.jittered(self.seed)
        energies, f_rl, f_own = binding_reference(s, LIGAND, tag, pos)
        e_ref, u_ref, f_ref = combine(energies, f_rl, f_own, lam)
        unit = max(1.0, 1e-3 * max(abs(x) for x in energies))
        e, u, f, terms = self.ene.item(), self.u.item(), self.frc.cpu().numpy(), self.terms.cpu().numpy()
        note(family, f"jittered({self.seed}) {kind} u (scale {unit:.3f})", abs(u - u_ref))
        assert abs(u - u_ref) < TIGHT * unit, f"u differs by {abs(u - u_ref):.3e}"
        if kind == "D":
            d_ref, du_ref, _ = binding_decomposition_reference(s, LIGAND, tag, pos)
            worst = np.abs(terms - d_ref).max(axis=1)
            note(family, f"jittered({self.seed}) D planes {worst}", worst.max())
            assert worst.max() < TIGHT, f"D differs by {worst} (planes cavity, vdw, gb_self, gb_pair)"
            assert abs(terms.sum() - u) < TIGHT * unit, f"D.sum() {terms.sum()!r} is not u {u!r}"
            assert abs(u - du_ref) < TIGHT * unit
            assert (f == SENTINEL).all()
            return
        note(family, f"jittered({self.seed}) {kind} E_lambda", abs(e - e_ref))
        assert abs(e - e_ref) < TIGHT * unit, f"E_lambda differs by {abs(e - e_ref):.3e}"
        if kind == "F":
            note(family, f"jittered({self.seed}) F forces", np.abs(f - f_ref).max())
            assert np.abs(f - f_ref).max() < TIGHT, f"forces differ by {np.abs(f - f_ref).max():.3e}"
        else:
            assert (f == SENTINEL).all()
        assert not terms.any()


def settled_binding(torch, s, lam):
    force = P.AGBNPForce.from_arrays(*s.params(), version=1)
    b = P.BindingEnergy(force, LIGAND, device=0)
    stream = _stream(torch)
    outs = [BindingOut(torch, s, seed) for seed in (0, 1)]
    torch.cuda.synchronize()
    for o in outs:
        o.call("F", b, lam, stream)
    assert b.finish(stream) == 0, b.withheld()
    assert [int(b.member(m).scalar("variant")) for m in range(3)] == [0, 0, 0]
    return b


def member_states(b):
    return [state(b.member(m)) for m in range(3)]


@pytest.mark.parametrize("which", ["complex", "ligand"])
def test_a_binding_with_a_healing_member(gpu_required, systems, five_groups, which):
    """engine_binding.hip: a group of three members of very different sizes (272, 256 and 16 atoms) between the gather and the
    combine launch.  The complex frozen -- the largest grid -- or the ligand -- the smallest: execute_device at lambda = 0.35,
    energy_device and decompose_device queued; E_lambda, u, the forces and D[t][i] are the binding restatements', D sums to u."""
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    stream = _stream(torch)
    lam = 0.35
    b = settled_binding(torch, s, lam)
    system_of = {"complex": s, "receptor": s.subset(b.receptor_atoms), "ligand": s.subset(b.ligand_atoms)}
    freeze_packing(b.member(which), system_of[which].nheavy)
    seeds = (2, 3, 4)
    outs = [BindingOut(torch, s, seed, 0.0 if kind == "F" else SENTINEL) for seed, kind in zip(seeds, "FED")]
    torch.cuda.synchronize()
    gens = member_states(b)
    for o, kind in zip(outs, "FED"):
        o.call(kind, b, lam, stream)
    assert b.finish(stream) == 0, (b.withheld(), [int(b.member(m).scalar("overflow_kinds")) for m in range(3)])
    assert b.withheld() == []
    assert member_states(b) == gens
    assert [int(b.member(m).scalar("group_members")) for m in range(3)] == [3, 3, 3]
    healed = {name: int(b.member(name).scalar("healed_forests")) for name in system_of}
    print(f"binding with the {which} frozen: healed_forests {healed}")
    x = system_of[which]
    if which == "complex":
        assert healed[which] == healed_through_execute_device(torch, s, 1, seeds, (0, 1))
    else:  # (the twin's geometries: the ligand's atoms of the complex's)
        twin = kernel_of(x.params())
        sub = lambda seed: s.jittered(seed)[b.ligand_atoms]  # noqa: E731
        dev = torch.device("cuda:0")
        pos = torch.tensor(np.stack([sub(seed) for seed in (0, 1) + seeds]), dtype=torch.float64, device=dev).contiguous()
        frc, ene = torch.zeros((x.n, 3), dtype=torch.float64, device=dev), torch.zeros((1,), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        for i in (0, 1):
            twin.execute_device(pos[i].data_ptr(), frc.data_ptr(), ene.data_ptr(), stream)
        assert twin.finish(stream) == 0
        freeze_packing(twin, x.nheavy)
        for i in (2, 3, 4):
            twin.execute_device(pos[i].data_ptr(), frc.data_ptr(), ene.data_ptr(), stream)
        assert twin.finish(stream) == 0
        assert healed[which] == int(twin.scalar("healed_forests"))
    assert healed[which] > 0
    assert [healed[name] for name in system_of if name != which] == [0, 0]
    for o, kind in zip(outs, "FED"):
        o.check(f"binding, {which} frozen", kind, lam)


def test_a_binding_group_with_one_healing_binding(gpu_required, systems, five_groups):
    """Two trpcage bindings in one binding_execute_group call, the complex of the SECOND one frozen: six members in one launch
    set, the healing one in the middle of the grid; both bindings' E_lambda, u and forces are the restatement's."""
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    stream = _stream(torch)
    lams = [0.35, 0.6]
    bindings = [settled_binding(torch, s, lam) for lam in lams]
    freeze_packing(bindings[1].member("complex"), s.nheavy)
    outs = [BindingOut(torch, s, seed) for seed in (2, 3)]
    lam = torch.tensor(lams, dtype=torch.float64, device=torch.device("cuda:0"))
    torch.cuda.synchronize()
    gens = [member_states(b) for b in bindings]
    ptrs = lambda name: [getattr(o, name).data_ptr() for o in outs]  # noqa: E731
    P.binding_execute_group(bindings, ptrs("pos"), lam.data_ptr(), ptrs("frc"), ptrs("ene"), ptrs("u"), stream)
    assert [b.finish(stream) for b in bindings] == [0, 0], [b.withheld() for b in bindings]
    assert [member_states(b) for b in bindings] == gens
    assert [[int(b.member(m).scalar("group_members")) for m in range(3)] for b in bindings] == [[6, 6, 6]] * 2
    healed = [[int(b.member(m).scalar("healed_forests")) for m in range(3)] for b in bindings]
    print("binding group: healed_forests", healed)
    assert healed[1][0] == healed_through_execute_device(torch, s, 1, (3,), (0, 1))
    assert healed[0] == [0, 0, 0] and healed[1][1:] == [0, 0]
    for o, x in zip(outs, lams):
        o.check("binding group, second complex frozen", "F", x)


# ---- 8. deterministic mode -----------------------------------------------------------------------------------------------------
def test_deterministic_mode_is_bit_identical_across_a_healed_packing(gpu_required, systems, five_groups):
    """include/agbnp_hip.h promises the deterministic mode's results bit-identical from run to run whatever the packing; a healed
    evaluation sums every slot's energy and every atom's self volume over another split into sets than any planned packing does.
    A frozen context and a healthy twin over three geometries: energies and forces of execute_device and the planes of
    decompose_device are the same BITS; both are the oracle's."""
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    stream = _stream(torch)
    k, twin = kernel_of(s.params(), 1, "deterministic"), kernel_of(s.params(), 1, "deterministic")
    for x in (k, twin):
        settle(torch, x, s, (0, 1))
    freeze_packing(k, s.nheavy)
    seeds = (2, 3, 4)
    full, tfull = ([Out(torch, s, seed) for seed in seeds] for _ in range(2))
    dec, tdec = ([Out(torch, s, seed, SENTINEL) for seed in seeds] for _ in range(2))
    torch.cuda.synchronize()
    gen = state(k)
    for x, fs, ds in ((k, full, dec), (twin, tfull, tdec)):
        for o in fs:
            o.single("F", x, stream)
        for o in ds:
            o.single("D", x, stream)
    assert k.finish(stream) == 0, (list(k.withheld()), int(k.scalar("overflow_kinds")))
    assert twin.finish(stream) == 0
    assert state(k) == gen
    assert int(k.scalar("healed_forests")) == healed_through_execute_device(torch, s, 1, seeds + seeds, (0, 1), "deterministic")
    assert int(twin.scalar("healed_forests")) == 0
    differing = []
    for kind, mine, theirs in (("F", full, tfull), ("D", dec, tdec)):
        for o, t in zip(mine, theirs):
            check_member("deterministic mode", kind, o, 1, t)
            (e, f, terms), (te, tf, tt) = o.result(), t.result()
            if e != te:
                differing.append((kind, o.seed, "energy", e - te))
            for name, a, b in (("forces", f, tf), ("planes", terms, tt)):
                if not np.array_equal(a, b):
                    where = np.argwhere(a != b)
                    differing.append((kind, o.seed, name, len(where), where[:8].tolist(), float(np.abs(a - b).max())))
    assert not differing, f"a healed evaluation differs in its bits from the planned packing's: {differing}"
