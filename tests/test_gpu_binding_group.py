"""GPU box: binding groups (include/agbnp_hip.h: agbnp_hip_binding_execute_group and its kin) -- several bindings
evaluated in one call on one gather launch, the members' evaluations as replica groups and one combine launch that takes every
binding's lambda from device memory.  The reference and the tolerances are those of tests/test_gpu_binding.py: the NumPy
combination of three CPU oracles (tests/binding_restatement.py), one evaluation per partition and geometry shared through that
module's REFS, and its `check` (TIGHT per member evaluation and the weights of the combination, times the count of evaluations
added)."""
import os
import subprocess

import numpy as np
import pytest

import openmm_agbnp_plugin_amd as P
from tests.binding_restatement import combine
from tests.edge_systems import edge_systems
from tests.gpu_helpers import five_groups  # noqa: F401
from tests.test_gpu_binding import EDGES, LAMBDAS, Buffers, _binding, _moved, check, reference

pytestmark = pytest.mark.gpu

LIGAND = list(range(16))  # of trpcage
POOL = []  # trpcage bindings (ligand 0 .. 15, version 1, reference mode), made once and only ever moved between jitter steps


def pool(systems, count):
    while len(POOL) < count:
        POOL.append(_binding(systems("trpcage"), LIGAND))
    return POOL[:count]


def lambdas_of(count):
    return [LAMBDAS[(k + k // 4) % 4] for k in range(count)]


class Group:
    """The caller's side of a binding group: one Buffers per binding, the lambdas as a device tensor."""

    def __init__(self, torch, bindings, lams, fill=(0.0, 0.0, 0.0)):
        self.torch, self.bindings, self.lams = torch, list(bindings), [float(x) for x in lams]
        self.bufs = [Buffers(torch, b.numParticles, fill) for b in self.bindings]
        self.lam = torch.tensor(self.lams, dtype=torch.float64, device=torch.device("cuda:0"))
        self.stream = self.bufs[0].stream
        torch.cuda.synchronize()

    def load(self, geoms):
        for buf, geom in zip(self.bufs, geoms):
            buf.load(geom)

    def _p(self, name):
        return [getattr(buf, name).data_ptr() for buf in self.bufs]

    def execute(self):
        P.binding_execute_group(self.bindings, self._p("pos"), self.lam.data_ptr(), self._p("frc"), self._p("ene"), self._p("u"), self.stream)

    def energy(self):
        P.binding_energy_group(self.bindings, self._p("pos"), self.lam.data_ptr(), self._p("ene"), self._p("u"), self.stream)

    def finish(self):
        return [b.finish(self.stream) for b in self.bindings]

    def results(self):
        self.torch.cuda.synchronize()
        return [buf.result() for buf in self.bufs]

    def kinds(self):
        return [[int(b.member(m).scalar("last_evaluation_kind")) for m in range(3)] for b in self.bindings]


def members_sharing(bindings, scalar="group_members"):
    return [[int(b.member(m).scalar(scalar)) for m in range(3)] for b in bindings]


def expected_sharing(bindings):
    """Members of the same group call (one call where 3 K <= 16, else one per kind) with the same capacity variant."""
    variants = [[int(b.member(m).scalar("variant")) for m in range(3)] for b in bindings]
    one_call = 3 * len(bindings) <= 16
    want = []
    for k, row in enumerate(variants):
        want.append([sum(1 for j, other in enumerate(variants) for mm in range(3) if (one_call or mm == m) and other[mm] == row[m])
                     for m in range(3)])
    return want, variants


# ---- 1. parity with the restatement ----------------------------------------------------------------------------------
PARITY = {  # name -> (system, ligand atoms, version, bindings)
    "trpcage_K1": ("trpcage", LIGAND, 1, 1),
    "trpcage_K2": ("trpcage", LIGAND, 1, 2),
    "trpcage_K5": ("trpcage", LIGAND, 1, 5),
    "trpcage_K6": ("trpcage", LIGAND, 1, 6),
    "trpcage_K16": ("trpcage", LIGAND, 1, 16),
    "fixture264_K3": ("fixture264", list(range(200, 264)), 1, 3),
    "trpcage_v0_K2": ("trpcage", list(range(100, 130)), 0, 2),
}


@pytest.mark.parametrize("case", sorted(PARITY))
def test_parity_with_the_restatement(gpu_required, systems, five_groups, case):
    """Binding k at jittered(k % 4) with lambda_k spread over {0, 0.35, 1, 1.5}: the full form, then the energy-only form against
    a sentinel force buffer that stays bit-identical.  3 K <= 16: one group call over all members; beyond: one per kind."""
    torch = pytest.importorskip("torch")
    name, ligand, version, count = PARITY[case]
    s = systems(name)
    bindings = pool(systems, count) if (name, version) == ("trpcage", 1) else [_binding(s, ligand, version=version) for _ in range(count)]
    lams = lambdas_of(count)
    geoms = [s.jittered(k % 4) for k in range(count)]
    refs = [reference(s, ligand, f"jitter{k % 4}", geoms[k], version=version) for k in range(count)]
    g = Group(torch, bindings, lams)
    g.load(geoms)
    g.execute()
    assert g.finish() == [0] * count
    assert g.kinds() == [[0, 0, 0]] * count
    for k, got in enumerate(g.results()):
        check(got, refs[k], lams[k], what=f"{case} binding {k}")
    want, variants = expected_sharing(bindings)
    print(f"{case}: variants {variants}, launch-set sizes {members_sharing(bindings)}")
    assert members_sharing(bindings) == want
    sentinel = -123.456
    only = Group(torch, bindings, lams, fill=(0.0, 0.0, sentinel))
    only.load(geoms)
    only.energy()
    assert only.finish() == [0] * count
    assert all(kind in (1, 2) for row in only.kinds() for kind in row)
    for k, (e, u, f) in enumerate(only.results()):
        assert (only.bufs[k].frc == sentinel).all().item(), f"binding {k}: the energy-only form wrote a force"
        check((e, u, combine(*refs[k], lams[k])[2]), refs[k], lams[k], what=f"{case} binding {k} energy form")
    assert all(b.withheld() == [] for b in bindings)


# ---- 2. mixed systems in one call ------------------------------------------------------------------------------------
def test_bindings_of_different_complexes_in_one_call(gpu_required, systems, five_groups):
    """trpcage, a ligand strewn over size_129_257, size_1_33 with its heavy atom (versions 1 and 0: two launch sets at least) and
    the edge map of size_257_513 (the ligand is the last 257 atoms and ends one atom into a new 256-thread block): five grids of
    different sizes side by side in the gather and the combine launch."""
    torch = pytest.importorskip("torch")
    edges = edge_systems()
    heavy = np.flatnonzero(edges["size_1_33"].ishydrogen == 0).tolist()
    cases = [(systems("trpcage"), LIGAND, 1, "jitter1"), (edges["size_129_257"], list(range(0, 257, 3)), 1, "file"),
             (edges["size_1_33"], heavy, 1, "file"), (edges["size_257_513"], list(range(256, 513)), 1, "file"),
             (edges["size_1_33"], heavy, 0, "file")]
    bindings = [_binding(s, ligand, version=version) for s, ligand, version, _ in cases]
    geoms = [s.jittered(1) if tag == "jitter1" else s.pos for s, _, _, tag in cases]
    refs = [reference(s, ligand, tag, geom, version=version) for (s, ligand, version, tag), geom in zip(cases, geoms)]
    lams = [0.35, 1.5, 0.0, 0.35, 1.0]
    for fill in ((0.0, 0.0, 0.0), (2.0, 3.0, 1.0)):
        g = Group(torch, bindings, lams, fill)
        g.load(geoms)
        g.execute()
        assert g.finish() == [0] * len(cases)
        for k, got in enumerate(g.results()):
            check(got, refs[k], lams[k], fill=fill, what=f"mixed call, {cases[k][0].name} v{cases[k][2]}")
    g = Group(torch, bindings, lams)
    g.load(geoms)
    g.energy()
    assert g.finish() == [0] * len(cases)
    for k, (e, u, f) in enumerate(g.results()):
        assert not f.any()
        check((e, u, combine(*refs[k], lams[k])[2]), refs[k], lams[k], what=f"mixed energy call, {cases[k][0].name}")


# ---- 3. deterministic mode -------------------------------------------------------------------------------------------
def test_deterministic_mode_is_bit_identical_to_six_single_calls(gpu_required, systems, five_groups):
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    count = 6
    bindings = [_binding(s, LIGAND, mode="deterministic") for _ in range(count)]
    lams = lambdas_of(count)
    geoms = [s.jittered(k % 4) for k in range(count)]
    runs = []
    for _ in range(2):
        g = Group(torch, bindings, lams)
        g.load(geoms)
        g.execute()
        assert g.finish() == [0] * count
        runs.append(g.results())
    single = Group(torch, bindings, lams)
    single.load(geoms)
    for b, buf, lam in zip(bindings, single.bufs, lams):
        buf.execute(b, lam)
    assert single.finish() == [0] * count
    for k, (a, b, c) in enumerate(zip(runs[0], runs[1], single.results())):
        for other, what in ((b, "run to run"), (c, "against the single call")):
            assert a[0] == other[0] and a[1] == other[1] and np.array_equal(a[2], other[2]), f"binding {k} differs {what}"
        check(a, reference(s, LIGAND, f"jitter{k % 4}", geoms[k]), lams[k], what=f"deterministic binding {k}")


def _bits(*values):
    return [np.ascontiguousarray(v, dtype=np.float64).reshape(-1).view(np.uint64) for v in values]


@pytest.mark.parametrize("case", sorted(EDGES) + ["trpcage_0_15"])
def test_a_group_of_one_is_the_single_call_bit_for_bit(gpu_required, systems, five_groups, case):
    """The single and the group kernels are wrappers round ONE per-atom gather and ONE per-atom combine: at the shapes where a
    wrapper could index differently (one atom in the last workgroup, a ligand at either end, a strewn ligand, a receptor without
    a heavy atom) a group of one gives the single call's F_lambda, E_lambda and u bit for bit, in the deterministic mode (which
    is bit-identical from run to run, so a difference is the wrappers'), and so does the energy-only form, which writes no force."""
    torch = pytest.importorskip("torch")
    if case == "trpcage_0_15":
        s, ligand, version = systems("trpcage"), LIGAND, 1
    else:
        name, ligand, version = EDGES[case]
        s = edge_systems()[name]
        ligand = np.flatnonzero(s.ishydrogen == 0).tolist() if isinstance(ligand, str) else list(ligand)
    b = _binding(s, ligand, version=version, mode="deterministic")
    b.execute(s.pos, 0.35)  # (settles the capacity variants: the device calls below repeat nothing)
    sentinel = -123.456
    for form, fill in (("execute", (0.0, 0.0, 0.0)), ("energy", (0.0, 0.0, sentinel))):
        single = Buffers(torch, s.n, fill)
        single.load(s.pos)
        getattr(single, form)(b, 0.35)
        assert b.finish(single.stream) == 0
        torch.cuda.synchronize()
        g = Group(torch, [b], [0.35], fill)
        g.load([s.pos])
        getattr(g, form)()
        assert g.finish() == [0]
        for a, c, what in zip(_bits(*single.result()), _bits(*g.results()[0]), ("E_lambda", "u", "F_lambda")):
            assert np.array_equal(a, c), f"{case} {form}: {what} of a group of one is not the single call's"
        assert single.result()[0] != 0.0  # (an evaluation was added, not two withheld ones compared)
        if form == "energy":
            assert (single.frc == sentinel).all().item() and (g.bufs[0].frc == sentinel).all().item()
    assert b.withheld() == []


# ---- 4. launch sharing -----------------------------------------------------------------------------------------------
def test_members_share_launch_sets(gpu_required, systems, five_groups):
    """K = 5: one group call over 15 members; K = 6: one call per kind, six members each.  Members of one call that differ in
    capacity variant are different launch sets: then the count of same-variant members of the call is what scalar 19 says."""
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    for count, full in ((5, 15), (6, 6)):
        bindings = pool(systems, count)
        g = Group(torch, bindings, lambdas_of(count))
        g.load([s.jittered(k % 4) for k in range(count)])
        g.execute()
        assert g.finish() == [0] * count
        want, variants = expected_sharing(bindings)
        got = members_sharing(bindings)
        print(f"K = {count}: variants {variants}, scalar 19 {got}")
        assert got == want
        if len({v for row in variants for v in row}) == 1:
            assert got == [[full] * 3] * count
        assert all(n >= count for row in got for n in row)  # (same-kind members of one system share at least among themselves)


# ---- 5. lambda lives on the device -----------------------------------------------------------------------------------
def test_lambda_is_read_from_device_memory_when_the_combine_runs(gpu_required, systems, five_groups):
    """Two calls with ONE d_lambdas tensor whose contents a torch operation on the same stream changes in between, no host-side
    API call in between: the second call's sums follow the new values.  And two bindings that share one position buffer at
    lambda = 0 and 1 give the separated and the complex results."""
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    bindings = pool(systems, 2)
    pos = s.jittered(1)
    ref = reference(s, LIGAND, "jitter1", pos)
    g = Group(torch, bindings, [0.35, 1.5])
    g.load([pos, pos])
    new = torch.tensor([1.0, 0.0], dtype=torch.float64, device=torch.device("cuda:0"))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g.stream = side.cuda_stream
    with torch.cuda.stream(side):
        g.execute()
        g.lam.copy_(new)  # (a device-to-device copy enqueued on the stream)
        g.execute()
    assert g.finish() == [0, 0]
    for k, (old_lam, new_lam) in enumerate(((0.35, 1.0), (1.5, 0.0))):
        e, u, f = g.results()[k]
        first = combine(*ref, old_lam)
        check((e - first[0], u - first[1], f - first[2]), ref, new_lam, what=f"binding {k}: the second call at the new lambda")
    shared = Group(torch, bindings, [0.0, 1.0])
    shared.bufs[0].load(pos)
    pointers = [shared.bufs[0].pos.data_ptr()] * 2
    P.binding_execute_group(bindings, pointers, shared.lam.data_ptr(), shared._p("frc"), shared._p("ene"), shared._p("u"), shared.stream)
    assert shared.finish() == [0, 0]
    (e0, u0, f0), (e1, u1, f1) = shared.results()
    check((e0, u0, f0), ref, 0.0, what="shared positions, lambda 0")
    check((e1, u1, f1), ref, 1.0, what="shared positions, lambda 1")
    (e_rl, e_r, e_l), f_rl, f_own = ref
    assert abs(e0 - (e_r + e_l)) < 2e-7 * max(1.0, 1e-3 * abs(e_rl)) and abs(e1 - e_rl) < 1e-7 * max(1.0, 1e-3 * abs(e_rl))
    assert np.abs(f0 - f_own).max() < 1e-7 and np.abs(f1 - f_rl).max() < 1e-7


# ---- 6. the call adds ------------------------------------------------------------------------------------------------
def test_the_group_adds_and_takes_null_scalars(gpu_required, systems, five_groups):
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    bindings = pool(systems, 3)
    lams = [0.35, 1.0, 1.5]
    geoms = [s.jittered(k) for k in range(3)]
    refs = [reference(s, LIGAND, f"jitter{k}", geoms[k]) for k in range(3)]
    fill = (2.0, 3.0, 1.0)
    g = Group(torch, bindings, lams, fill)
    g.load(geoms)
    g.execute()
    g.execute()
    # NULL entries (E of binding 0, u of binding 1, both of binding 2), then NULL arrays
    part = Group(torch, bindings, lams)
    part.load(geoms)
    ene, u = part._p("ene"), part._p("u")
    P.binding_execute_group(bindings, part._p("pos"), part.lam.data_ptr(), part._p("frc"), [None, ene[1], None], [u[0], None, None], part.stream)
    none = Group(torch, bindings, lams)
    none.load(geoms)
    P.binding_execute_group(bindings, none._p("pos"), none.lam.data_ptr(), none._p("frc"), None, None, none.stream)
    only = Group(torch, bindings, lams)
    only.load(geoms)
    P.binding_energy_group(bindings, only._p("pos"), only.lam.data_ptr(), [None] + only._p("ene")[1:],
                           [only._p("u")[0], None, only._p("u")[2]], only.stream)
    assert g.finish() == [0, 0, 0]
    for k in range(3):
        e_ref, u_ref, f_ref = combine(*refs[k], lams[k])
        check(g.results()[k], refs[k], lams[k], count=2, fill=fill, what=f"binding {k}: two into filled buffers")
        e, uu, f = part.results()[k]
        assert (e == 0.0) == (k != 1) and (uu == 0.0) == (k != 0)
        check((e if k == 1 else e_ref, uu if k == 0 else u_ref, f), refs[k], lams[k], what=f"binding {k}: NULL entries")
        e, uu, f = none.results()[k]
        assert e == 0.0 and uu == 0.0
        check((e_ref, u_ref, f), refs[k], lams[k], what=f"binding {k}: NULL arrays")
        e, uu, f = only.results()[k]
        assert not f.any() and (e == 0.0) == (k == 0) and (uu == 0.0) == (k == 1)
        check((e if k != 0 else e_ref, uu if k != 1 else u_ref, f_ref), refs[k], lams[k], what=f"binding {k}: energy form, NULL entries")
    with pytest.raises(P.OpenMMException, match="both null"):
        P.binding_energy_group(bindings, only._p("pos"), only.lam.data_ptr(), [None, 1, 2], [None, 3, 4], only.stream)
    with pytest.raises(P.OpenMMException, match="both null"):
        P.binding_energy_group(bindings, only._p("pos"), only.lam.data_ptr(), None, None, only.stream)
    word = only._p("ene")[0]
    with pytest.raises(P.OpenMMException, match="the same"):
        P.binding_energy_group(bindings, only._p("pos"), only.lam.data_ptr(), [word, ene[1], ene[2]], [word, u[1], u[2]], only.stream)
    assert [b.finish() for b in bindings] == [0, 0, 0]


# ---- 7. all or nothing, per binding ----------------------------------------------------------------------------------
def test_a_withheld_binding_leaves_the_others_alone(gpu_required, systems, five_groups):
    """One binding of four has a ligand atom moved 0.1 nm between two calls: its three outputs are bit-unchanged, its finish() is 1
    and withheld() names the evaluation; the other three are right.  The repeat is right; with expect_jump() nothing is withheld."""
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    bindings = [_binding(s, LIGAND) for _ in range(4)]
    lams = lambdas_of(4)
    fill = (2.0, 3.0, 1.0)
    warm = Group(torch, bindings, lams)
    warm.load([s.pos] * 4)
    warm.execute()
    assert warm.finish() == [0, 0, 0, 0]
    index = 2
    heavy_ligand = [a for a in LIGAND if s.ishydrogen[a] == 0]
    moved = _moved(s, heavy_ligand[len(heavy_ligand) // 2])
    geoms = [moved if k == index else s.jittered(k) for k in range(4)]
    g = Group(torch, bindings, lams, fill)
    g.load(geoms)
    torch.cuda.synchronize()
    snap = g.bufs[index].snapshot()
    g.execute()
    assert g.finish() == [1 if k == index else 0 for k in range(4)]
    assert [b.withheld() for b in bindings] == [[0] if k == index else [] for k in range(4)]
    torch.cuda.synchronize()
    assert g.bufs[index].unchanged_since(snap)  # bit for bit
    for k in range(4):
        if k != index:
            check(g.results()[k], reference(s, LIGAND, f"jitter{k}", geoms[k]), lams[k], fill=fill, what=f"binding {k} beside the withheld one")
    rep = Group(torch, bindings, lams, fill)
    rep.load(geoms)
    rep.execute()  # the repeat: nothing of the withheld evaluation was left in the binding's own buffers
    assert rep.finish() == [0, 0, 0, 0] and all(b.withheld() == [] for b in bindings)
    check(rep.results()[index], reference(s, LIGAND, "moved_ligand", moved), lams[index], fill=fill, what="the repeat")
    moved2 = _moved(s, heavy_ligand[0], -0.1)
    geoms[index] = moved2
    fresh = Group(torch, bindings, lams)
    fresh.load(geoms)
    bindings[index].expect_jump()
    fresh.execute()
    assert fresh.finish() == [0, 0, 0, 0]
    check(fresh.results()[index], reference(s, LIGAND, "moved_ligand2", moved2), lams[index], what="behind the hint")
    # the energy form is gated the same way
    back = Group(torch, bindings, lams, fill)
    back.load([s.pos if k == index else geoms[k] for k in range(4)])
    torch.cuda.synchronize()
    snap = back.bufs[index].snapshot()
    back.energy()
    assert back.finish() == [1 if k == index else 0 for k in range(4)]
    torch.cuda.synchronize()
    assert back.bufs[index].unchanged_since(snap)


# ---- 8. queueing and the steady state --------------------------------------------------------------------------------
def test_twenty_queued_group_calls_and_steady_argument_blocks(gpu_required, systems, five_groups):
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    count, steps = 3, 20
    bindings = pool(systems, count)
    lams = [0.35, 1.0, 1.5]
    geoms = [s.jittered(step) for step in range(steps + count)]
    walk = torch.tensor(np.stack(geoms), dtype=torch.float64, device=torch.device("cuda:0"))
    g = Group(torch, bindings, lams)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()  # (the copies into the fixed position buffers and the evaluations are ordered on it)
    g.stream = side.cuda_stream
    writes = None
    with torch.cuda.stream(side):
        for step in range(steps):
            for k in range(count):
                g.bufs[k].pos.copy_(walk[step + k])
            g.execute()
            if step == 1:
                writes = members_sharing(bindings, "group_block_writes")
    assert g.finish() == [0] * count, [b.withheld() for b in bindings]
    assert members_sharing(bindings, "group_block_writes") == writes
    for k, (e, u, f) in enumerate(g.results()):
        total, worst = [0.0, 0.0, np.zeros((s.n, 3))], 0.0
        for step in range(steps):
            ref = reference(s, LIGAND, f"jitter{step + k}", geoms[step + k])
            for j, part in enumerate(combine(*ref, lams[k])):
                total[j] = total[j] + part
            worst = max(worst, max(abs(x) for x in ref[0]))
        unit = max(1.0, 1e-3 * worst)
        lam = lams[k]
        de, du, df = abs(e - total[0]), abs(u - total[1]), float(np.abs(f - total[2]).max())
        print(f"20 queued, binding {k}: |dE_lam| {de:.2e}  |du| {du:.2e}  max|dF| {df:.2e}")
        assert df < steps * 1e-7 * (abs(lam) + abs(1 - lam)) and de < steps * 1e-7 * (abs(lam) + 2 * abs(1 - lam)) * unit
        assert du < steps * 3e-7 * unit


# ---- 9. group and single calls interleaved ---------------------------------------------------------------------------
def test_group_and_single_calls_keep_every_log(gpu_required, systems, five_groups):
    """Single, group, group (binding 1's positions jump: withheld) and finish: every binding's log counts its own evaluations, and
    the withheld one is index 2 of binding 1 alone.  Then the repeat of binding 1 alone, a group call and finish: nothing."""
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    bindings = [_binding(s, LIGAND) for _ in range(2)]
    lams = [0.35, 1.0]
    heavy_ligand = [a for a in LIGAND if s.ishydrogen[a] == 0]
    moved = _moved(s, heavy_ligand[1])
    g = Group(torch, bindings, lams)
    side = torch.cuda.Stream()
    g.stream = side.cuda_stream
    for buf in g.bufs:
        buf.stream = g.stream
    torch.cuda.synchronize()
    added = [[], []]  # what reaches every binding's buffers: (tag, geometry)
    with torch.cuda.stream(side):
        def put(k, tag, geom):
            g.bufs[k].pos.copy_(torch.tensor(geom, dtype=torch.float64))
            return tag, geom
        for k in range(2):
            added[k].append(put(k, "file", s.pos))
            g.bufs[k].execute(bindings[k], lams[k])
        added[0].append(put(0, "jitter1", s.jittered(1)))
        added[1].append(put(1, "jitter2", s.jittered(2)))
        g.execute()
        put(1, "moved_ligand_b", moved)  # binding 1 jumps: its evaluation 2 is withheld
        added[0].append(put(0, "jitter2", s.jittered(2)))
        g.execute()
    assert g.finish() == [0, 1]
    assert bindings[0].withheld() == [] and bindings[1].withheld() == [2]
    with torch.cuda.stream(side):
        added[1].append(put(1, "moved_ligand_b", moved))
        g.bufs[1].execute(bindings[1], lams[1])  # the repeat, alone
        added[0].append(put(0, "jitter3", s.jittered(3)))
        g.execute()
        added[1].append(("moved_ligand_b", moved))
    assert g.finish() == [0, 0]
    assert bindings[0].withheld() == [] and bindings[1].withheld() == []
    for k in range(2):
        total = [0.0, 0.0, np.zeros((s.n, 3))]
        for tag, geom in added[k]:
            for j, part in enumerate(combine(*reference(s, LIGAND, tag, geom), lams[k])):
                total[j] = total[j] + part
        e, u, f = g.results()[k]
        count = len(added[k])
        ref = reference(s, LIGAND, "file", s.pos)
        unit = max(1.0, 1e-3 * max(abs(x) for x in ref[0]))
        assert np.abs(f - total[2]).max() < count * 1e-7 * (abs(lams[k]) + abs(1 - lams[k]))
        assert abs(e - total[0]) < count * 1e-7 * (abs(lams[k]) + 2 * abs(1 - lams[k])) * unit and abs(u - total[1]) < count * 3e-7 * unit


def test_single_and_group_calls_on_the_null_stream_are_ordered(gpu_required, systems, five_groups):
    """With a NULL stream a single call runs on ITS binding's complex's stream and a group call on the FIRST binding's: a single
    call on binding 1 queued directly in front of a group call of {binding 0, binding 1} -- no finish in between -- must have
    read binding 1's own position buffer before the group's gather overwrites it, and the reverse.  Five rounds of each order at
    alternating geometries, every call into buffers of its own: each sum is that of its own calls."""
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    bindings = [_binding(s, LIGAND) for _ in range(2)]
    lams = [0.35, 1.0]
    single_lam = 1.5
    rounds = 5
    for order in ("single first", "group first"):
        g = Group(torch, bindings, lams)
        single = Buffers(torch, s.n)
        assert g.stream in (0, None) and single.stream in (0, None)  # (the library's NULL stream)
        tags = {"group0": [], "group1": [], "single": []}
        for j in range(rounds):
            steps = (j % 4, (j + 1) % 4, (j + 2) % 4)  # binding 0 in the group, binding 1 in the group, binding 1 alone
            g.load([s.jittered(steps[0]), s.jittered(steps[1])])
            single.load(s.jittered(steps[2]))
            if order == "single first":
                single.execute(bindings[1], single_lam)
                g.execute()
            else:
                g.execute()
                single.execute(bindings[1], single_lam)
            for key, step in zip(("group0", "group1", "single"), steps):
                tags[key].append(step)
            torch.cuda.synchronize()  # (the next round's loads must not overtake this round's calls: not what is tested)
        assert g.finish() == [0, 0], [b.withheld() for b in bindings]
        for key, got, lam in (("group0", g.results()[0], lams[0]), ("group1", g.results()[1], lams[1]), ("single", single.result(), single_lam)):
            total = [0.0, 0.0, np.zeros((s.n, 3))]
            for step in tags[key]:
                for j, part in enumerate(combine(*reference(s, LIGAND, f"jitter{step}", s.jittered(step)), lam)):
                    total[j] = total[j] + part
            ref = reference(s, LIGAND, "jitter0", s.jittered(0))
            unit = max(1.0, 1e-3 * max(abs(x) for x in ref[0]))
            de, du, df = abs(got[0] - total[0]), abs(got[1] - total[1]), float(np.abs(got[2] - total[2]).max())
            print(f"NULL stream, {order}, {key}: |dE_lam| {de:.2e}  |du| {du:.2e}  max|dF| {df:.2e}")
            assert df < rounds * 1e-7 * (abs(lam) + abs(1 - lam)) and de < rounds * 1e-7 * (abs(lam) + 2 * abs(1 - lam)) * unit
            assert du < rounds * 3e-7 * unit


# ---- 10. refusals ----------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_anything_is_launched(gpu_required, systems, five_groups):
    """Overlapping force spans, a shared energy word, a shared u word, an energy word inside another binding's forces, a binding
    given twice, count 17, a NULL position or force pointer: each is refused, nothing is launched -- scalar 20 of every member
    still says that its last evaluation was the energy-only one -- and no output changes."""
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    bindings = pool(systems, 3)
    lams = [0.35, 1.0, 1.5]
    g = Group(torch, bindings, lams, (2.0, 3.0, 1.0))
    g.load([s.pos] * 3)
    g.energy()
    assert g.finish() == [0, 0, 0]
    kinds = g.kinds()
    assert all(kind in (1, 2) for row in kinds for kind in row)
    torch.cuda.synchronize()
    snaps = [buf.snapshot() for buf in g.bufs]
    pos, frc, ene, u, lam = g._p("pos"), g._p("frc"), g._p("ene"), g._p("u"), g.lam.data_ptr()
    big = torch.zeros((2 * s.n, 3), dtype=torch.float64, device=torch.device("cuda:0"))
    second = big.data_ptr() + 8 * (3 * s.n - 1)  # the last word of the span [3N] that starts at `big`
    E = P.OpenMMException
    with pytest.raises(E, match="overlap"):
        P.binding_execute_group(bindings, pos, lam, [big.data_ptr(), second, frc[2]], ene, u, g.stream)
    with pytest.raises(E, match="overlap"):
        P.binding_execute_group(bindings, pos, lam, [second, frc[1], big.data_ptr()], ene, u, g.stream)
    with pytest.raises(E, match="overlap"):
        P.binding_execute_group(bindings, pos, lam, frc, [ene[0], ene[0], ene[2]], u, g.stream)
    with pytest.raises(E, match="overlap"):
        P.binding_execute_group(bindings, pos, lam, frc, ene, [u[0], u[1], u[0]], g.stream)
    with pytest.raises(E, match="overlap"):
        P.binding_execute_group(bindings, pos, lam, frc, [ene[0], frc[2] + 8 * 5, ene[2]], u, g.stream)
    with pytest.raises(E, match="overlap"):
        P.binding_execute_group(bindings, pos, lam, frc, [ene[0], u[2], ene[2]], u, g.stream)
    with pytest.raises(E, match="overlap"):
        P.binding_energy_group(bindings, pos, lam, [ene[0], ene[0], ene[2]], u, g.stream)
    with pytest.raises(E, match="null pointer"):
        P.binding_execute_group(bindings, [pos[0], None, pos[2]], lam, frc, ene, u, g.stream)
    with pytest.raises(E, match="null pointer"):
        P.binding_execute_group(bindings, pos, lam, [frc[0], frc[1], None], ene, u, g.stream)
    # what the Python wrapper would stop itself goes to the library directly
    import ctypes as C
    from openmm_agbnp_plugin_amd import _lib
    lib = _lib.load()
    vp3 = C.c_void_p * 3
    arr = lambda ptrs: vp3(*ptrs)  # noqa: E731
    twice = vp3(bindings[0]._h, bindings[1]._h, bindings[0]._h)
    assert lib.agbnp_hip_binding_execute_group(twice, 3, arr(pos), lam, arr(frc), arr(ene), arr(u), g.stream) == _lib.ERR_INVALID_ARGUMENT
    assert "twice" in _lib.last_error(None)
    many = (C.c_void_p * 17)(*[bindings[k % 3]._h for k in range(17)])
    p17 = lambda ptrs: (C.c_void_p * 17)(*[ptrs[k % 3] for k in range(17)])  # noqa: E731
    assert lib.agbnp_hip_binding_execute_group(many, 17, p17(pos), lam, p17(frc), p17(ene), p17(u), g.stream) == _lib.ERR_INVALID_ARGUMENT
    assert "1 to 16" in _lib.last_error(None)
    assert lib.agbnp_hip_binding_execute_group(many, 0, p17(pos), lam, p17(frc), p17(ene), p17(u), g.stream) == _lib.ERR_INVALID_ARGUMENT
    assert lib.agbnp_hip_binding_execute_group(arr([b._h for b in bindings]), 3, arr(pos), None, arr(frc), arr(ene), arr(u), g.stream) == _lib.ERR_INVALID_ARGUMENT
    torch.cuda.synchronize()
    assert g.kinds() == kinds
    assert all(buf.unchanged_since(snap) for buf, snap in zip(g.bufs, snaps))
    assert g.finish() == [0, 0, 0]  # (nothing was enqueued)
    g.execute()  # and the bindings go on
    assert g.finish() == [0, 0, 0]
    ref = reference(s, LIGAND, "file", s.pos)
    for k in range(3):
        e, uu, f = g.results()[k]
        first = combine(*ref, lams[k])
        check((e - first[0], uu - first[1], f), ref, lams[k], fill=(2.0, 3.0, 1.0), what=f"binding {k} behind the refusals")


def test_the_group_calls_refuse_a_stream_capture(gpu_required, systems, five_groups):
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    bindings = pool(systems, 2)
    g = Group(torch, bindings, [0.35, 1.0])
    g.load([s.pos, s.pos])
    g.execute()
    assert g.finish() == [0, 0]
    first = g.results()
    marker = torch.zeros((1,), dtype=torch.float64, device=torch.device("cuda:0"))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        marker.fill_(1.0)
        g.stream = torch.cuda.current_stream().cuda_stream
        with pytest.raises(P.OpenMMException, match="captur"):
            g.execute()
        with pytest.raises(P.OpenMMException, match="captur"):
            g.energy()
    marker.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert marker.item() == 1.0
    g.stream = g.bufs[0].stream
    for a, b in zip(g.results(), first):
        assert a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2])  # nothing was launched
    g.execute()  # the bindings go on as before
    assert g.finish() == [0, 0]
    ref = reference(s, LIGAND, "file", s.pos)
    for k, lam in enumerate((0.35, 1.0)):
        check(g.results()[k], ref, lam, count=2, what=f"binding {k} behind the refused capture")


# ---- 11. host forms --------------------------------------------------------------------------------------------------
def test_the_host_forms_repeat_a_withheld_binding_and_carry_device_evaluations(gpu_required, systems, five_groups):
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    bindings = [_binding(s, LIGAND) for _ in range(3)]
    lams = [0.35, 1.0, 1.5]
    geoms = [s.jittered(k) for k in range(3)]
    refs = [reference(s, LIGAND, f"jitter{k}", geoms[k]) for k in range(3)]
    forces = [np.full((s.n, 3), 1.0) for _ in range(3)]
    e, u = P.binding_execute_group_host(bindings, geoms, lams, forces)
    for k in range(3):
        check((e[k], u[k], forces[k]), refs[k], lams[k], fill=(0.0, 0.0, 1.0), what=f"host form, binding {k}")
    e, u = P.binding_energy_group_host(bindings, geoms, lams)
    for k in range(3):
        check((e[k], u[k], combine(*refs[k], lams[k])[2]), refs[k], lams[k], what=f"host energy form, binding {k}")
    # binding 1 jumps: it is repeated inside, alone
    heavy = np.flatnonzero(s.ishydrogen == 0)
    moved = _moved(s, int(heavy[len(heavy) // 2]))
    geoms[1] = moved
    refs[1] = reference(s, LIGAND, "moved_host", moved)
    forces = [np.zeros((s.n, 3)) for _ in range(3)]
    e, u = P.binding_execute_group_host(bindings, geoms, lams, forces)
    for k in range(3):
        check((e[k], u[k], forces[k]), refs[k], lams[k], what=f"host form across a jump, binding {k}")
    geoms[1] = s.jittered(1)
    refs[1] = reference(s, LIGAND, "jitter1", geoms[1])
    e, u = P.binding_energy_group_host(bindings, geoms, lams)
    for k in range(3):
        check((e[k], u[k], combine(*refs[k], lams[k])[2]), refs[k], lams[k], what=f"host energy form across a jump, binding {k}")
    # a device evaluation that is withheld and unfinished when a host form harvests the logs: the next finish reports it
    g = Group(torch, bindings, lams, (2.0, 3.0, 1.0))
    g.load([geoms[0], moved, geoms[2]])
    torch.cuda.synchronize()
    snap = g.bufs[1].snapshot()
    g.execute()
    e, u = P.binding_energy_group_host(bindings, geoms, lams)
    for k in range(3):
        check((e[k], u[k], combine(*refs[k], lams[k])[2]), refs[k], lams[k], what=f"host form behind an unfinished group call, binding {k}")
    assert g.finish() == [0, 1, 0] and bindings[1].withheld() == [0]
    torch.cuda.synchronize()
    assert g.bufs[1].unchanged_since(snap)
    with pytest.raises(P.OpenMMException, match="finite"):
        P.binding_energy_group_host(bindings, geoms, [0.0, float("inf"), 1.0])


# ---- 12. modes -------------------------------------------------------------------------------------------------------
def test_members_that_run_their_own_launches(gpu_required, systems, monkeypatch):
    torch = pytest.importorskip("torch")
    monkeypatch.setenv("AGBNP_HIP_FIVE_LAUNCHES", "1")
    monkeypatch.setenv("AGBNP_HIP_GROUP_LAUNCHES", "0")
    s = systems("trpcage")
    for count in (2, 6):
        bindings = [_binding(s, LIGAND) for _ in range(count)]
        lams = lambdas_of(count)
        geoms = [s.jittered(k % 4) for k in range(count)]
        g = Group(torch, bindings, lams)
        g.load(geoms)
        g.execute()
        assert g.finish() == [0] * count
        for k, got in enumerate(g.results()):
            check(got, reference(s, LIGAND, f"jitter{k % 4}", geoms[k]), lams[k], what=f"group launches off, K = {count}, binding {k}")
        assert members_sharing(bindings) == [[0, 0, 0]] * count


def test_fast_mode_with_a_cutoff(gpu_required, systems, five_groups):
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    bindings = [_binding(s, LIGAND, mode="fast", cutoff=1.0) for _ in range(2)]
    ref = reference(s, LIGAND, "file", s.pos, cutoff=1.0)
    g = Group(torch, bindings, [0.35, 1.0])
    g.load([s.pos, s.pos])
    g.execute()
    assert g.finish() == [0, 0]
    for k, lam in enumerate((0.35, 1.0)):
        check(g.results()[k], ref, lam, what=f"fast mode, binding {k}")
    e, u = P.binding_energy_group_host(bindings, [s.pos, s.pos], [0.35, 1.0])
    for k, lam in enumerate((0.35, 1.0)):
        check((e[k], u[k], combine(*ref, lam)[2]), ref, lam, what=f"fast mode, host energy form, binding {k}")


# ---- 13. the C++ mirror ----------------------------------------------------------------------------------------------
def test_cpp_mirror_runs_a_binding_group(gpu_required, systems, five_groups, tmp_path):
    """tests/cxx/TestHipBindingGroup.cpp through cpp/AGBNPForce.h."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(root, "openmm_agbnp_plugin_amd")
    exe = str(tmp_path / "TestHipBindingGroup")
    subprocess.run(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    os.path.join(root, "tests", "cxx", "TestHipBindingGroup.cpp"), "-o", exe, os.path.join(libdir, "libagbnp_hip.so"),
                    "-L/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    x = systems("trpcage")
    path = tmp_path / "trpcage.txt"
    r, g, a, q, h = x.params()
    np.savetxt(path, np.column_stack([r, g, a, q, np.asarray(h, dtype=float), x.pos]), fmt="%.17g")
    out = subprocess.run([exe, str(path), "16"], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
