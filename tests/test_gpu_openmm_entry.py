"""GPU box: agbnp_hip_execute_openmm -- the entry point the OpenMM glue calls -- on the paths that had only run under
agbnp_hip_execute_device: forests healed inside the tree launch with the positions in an OpenMM context's posq (the POSQ branches
of csrc/tree_bodies.h: a rebuilt set's roots and the parts of a lone subtree find their slots through hslot), healing inside a
replayed graph (the device names the evaluation's set: k_tree_pseudo reads the spare forests behind the rebase), a captured
evaluation of this entry point (the DEV + POSQ instantiations of the cavity kernel), the POSQ kernels of the larger LDS stores, the
two entry points mixed around a captured graph (the words beside the work-slot rows hold slots for one and atom indices for the
other: agbnp_hip_generation() must say so), and the sequence of a long step and a reorder that tests/test_openmm_glue.py replays
through the glue.  The reference is the CPU oracle at the positions the engine sees (ReferenceAGBNPKernels.cpp:274-795); the
tolerances are those of tests/gpu_helpers.py and of test_the_openmm_entry_point_runs_in_the_mode."""
import numpy as np
import pytest

import openmm_agbnp_plugin_amd as P
from oracle import Oracle
from tests.gpu_helpers import TIGHT, Buffers, close, cluster, energy_close, execute_group, freeze_packing
from tests.gpu_helpers import five  # noqa: F401
from tests.openmm_context import ENERGY_SLOT, OpenMMContext, protocol_geometries

pytestmark = pytest.mark.gpu


def _kernel(s):
    k = P.HipCalcAGBNPForceKernel(device=0)
    k.initialize(P.AGBNPForce.from_arrays(*s.params(), version=1))
    return k


def _close(what, e, f, eo, fo, evaluations=1):
    """execute_device's buffers against the oracle's sums: TIGHT per evaluation (energy: energy_close's scaling)."""
    print(f"{what}: {evaluations} evaluation(s)  |dE|={abs(e - eo):.3e}  max|dF|={np.abs(f - fo).max():.3e}")
    energy_close(e, eo, evaluations * TIGHT)
    assert np.abs(f - fo).max() < evaluations * TIGHT, f"forces differ by {np.abs(f - fo).max():.3e}"


class _DeviceBuffers:
    """Positions, forces and energy of agbnp_hip_execute_device at addresses that stay (a captured graph freezes them)."""

    def __init__(self, torch, n):
        dev = torch.device("cuda:0")
        self.torch = torch
        self.pos = torch.zeros((n, 3), dtype=torch.float64, device=dev)
        self.frc = torch.zeros((n, 3), dtype=torch.float64, device=dev)
        self.ene = torch.zeros((1,), dtype=torch.float64, device=dev)

    def load(self, geom):
        self.pos.copy_(self.torch.tensor(geom, dtype=self.torch.float64))

    def clear(self):
        self.frc.zero_()
        self.ene.zero_()

    def enqueue(self, k, stream=None):
        stream = self.torch.cuda.current_stream().cuda_stream if stream is None else stream
        k.execute_device(self.pos.data_ptr(), self.frc.data_ptr(), self.ene.data_ptr(), stream)

    def result(self):
        self.torch.cuda.synchronize()
        return self.ene.item(), self.frc.cpu().numpy()


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("precision", ["double", "mixed"])
def test_overfull_forests_are_healed_through_the_openmm_entry(gpu_required, systems, five, precision):
    """The protocol of test_overfull_forests_are_healed_inside_the_tree_launch with the positions in a context's posq, shuffled and
    padded: 1dwc, a packing frozen at eight whole subtrees per forest, not one of the 261 forests fits its store.  The workgroups
    build them again in halves; the roots of the rebuilt sets are read at their SLOTS (tree_bodies.h: my_atom through A.hslot).
    Nothing is withheld, the sums of five queued geometries are the oracle's, no variant is raised, the chain stays five launches."""
    torch = pytest.importorskip("torch")
    s = systems("1dwc")
    k = _kernel(s)
    ctx = OpenMMContext(torch, s.n, precision, Oracle(*s.params(), version=1))
    stream = _stream(torch)
    geoms = [s.jittered(step) for step in range(5)]
    keep = ctx.run(k, geoms[:2], expect=False)[0]  # settle on the engine's own packing
    assert k.finish(stream) == 0
    assert int(k.scalar("launches")) == 5
    nf = freeze_packing(k, s.nheavy)
    ctx.clear()
    gen = k.generation()
    keep, we, wf = ctx.run(k, geoms)
    assert k.finish(stream) == 0, (list(k.withheld()), int(k.scalar("overflow_kinds")))
    assert int(k.scalar("healed_forests")) >= 5 * nf
    ctx.check(we, wf, 5, f"healing through execute_openmm ({precision})")
    assert int(k.scalar("variant")) == 0 and k.generation() == gen
    assert int(k.scalar("launches")) == 5


def test_a_lone_subtree_is_built_in_four_parts_through_the_openmm_entry(gpu_required, systems, five):
    """The 2clr case of test_a_lone_subtree_beyond_the_store_is_built_in_four_parts_at_once through a double-precision context in a
    shuffled order: a fresh context meets subtrees of more than 432 nodes one per work slot and builds them as the four parts of a
    four-way share, every part's root read at the subtree's slot (tree_bodies.h: the part_of_four roots through A.hslot).  Four
    geometries queued before anybody reads the log: none withheld, the oracle's sums."""
    torch = pytest.importorskip("torch")
    s = systems("2clr")
    k = _kernel(s)
    ctx = OpenMMContext(torch, s.n, "double", Oracle(*s.params(), version=1))
    stream = _stream(torch)
    geoms = [s.jittered(40 + step) for step in range(4)]
    keep = ctx.run(k, geoms, expect=False)[0]
    assert k.finish(stream) == 0, (list(k.withheld()), int(k.scalar("overflow_kinds")))
    assert int(k.scalar("healed_forests")) >= 1
    assert int(k.scalar("max_subtree_nodes")) > 432
    ctx.check(*ctx.expected(geoms), 4, "a lone subtree in four parts through execute_openmm")


def test_forests_are_healed_inside_a_replayed_graph(gpu_required, systems, five):
    """Healing where the DEVICE names the evaluation's set of accumulators (a context that has been captured: the DEV
    instantiations; k_tree_pseudo reads the count of spare forests behind the rebase): 1dwc through execute_device, settled, the
    packing frozen at eight subtrees per forest, ONE evaluation captured and replayed on four geometries, each replay the oracle's."""
    torch = pytest.importorskip("torch")
    s = systems("1dwc")
    k = _kernel(s)
    oracle = Oracle(*s.params(), version=1)
    buf = _DeviceBuffers(torch, s.n)
    for step in (0, 1):  # settle, outside the capture
        buf.load(s.jittered(step))
        buf.enqueue(k)
    assert k.finish(_stream(torch)) == 0
    freeze_packing(k, s.nheavy)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        buf.clear()
        buf.enqueue(k)
    gen = k.generation()
    for step in (2, 3, 4, 5):
        geom = s.jittered(step)
        buf.load(geom)
        g.replay()
        e, f = buf.result()
        _close(f"healing in a replayed graph, replay {step - 2}", e, f, *oracle.execute(geom))
    assert k.finish(_stream(torch)) == 0, (list(k.withheld()), int(k.scalar("overflow_kinds")))
    assert int(k.scalar("healed_forests")) > 0
    assert int(k.scalar("variant")) == 0 and k.generation() == gen


def test_a_captured_openmm_evaluation_replays(gpu_required, systems, five):
    """k_tree_cavity_five<..., DEV, POSQ>: selected only when a context that has been captured runs through the OpenMM entry.
    trpcage, double: one execute_openmm captured on buffers whose addresses stay, replayed on five geometries copied in between,
    one eager execute_openmm between two replays; each is the oracle's; five launches."""
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    k = _kernel(s)
    oracle = Oracle(*s.params(), version=1)
    ctx = OpenMMContext(torch, s.n, "double", oracle)
    for step in range(3):
        ctx.load(s.jittered(step))
        ctx.enqueue(k)
    assert k.finish(_stream(torch)) == 0
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ctx.clear()
        ctx.enqueue(k)
    for step in (5, 6, 7, 8, 9):
        seen = ctx.load(s.jittered(step))
        g.replay()
        ctx.check(*oracle.execute(seen), 1, f"captured execute_openmm, replay {step - 5}")
        if step == 7:
            keep, we, wf = ctx.run(k, [s.jittered(27)])
            assert k.finish(_stream(torch)) == 0
            ctx.check(we, wf, 1, "eager execute_openmm between two replays")
    assert k.finish(_stream(torch)) == 0
    assert int(k.scalar("launches")) == 5


@pytest.mark.parametrize("precision", ["double", "mixed"])
@pytest.mark.parametrize("spacing,variant", [(0.24, 2), (0.22, 3)])
def test_the_openmm_entry_is_exact_on_the_larger_stores(gpu_required, five, monkeypatch, spacing, variant, precision):
    """The POSQ kernels of the larger LDS stores (tree_kernels.hip: one instantiation per capacity variant): the first two clusters
    of test_every_capacity_variant_is_exact through execute_openmm.  The variant climbs the way a caller sees it: finish() reports
    the evaluation withheld, nothing has arrived, it is enqueued again; then two jittered evaluations on the settled variant."""
    torch = pytest.importorskip("torch")
    monkeypatch.setenv("AGBNP_HIP_SPLIT_FIT", "0")
    sysm = cluster(150, spacing, 1)
    k = _kernel(sysm)
    ctx = OpenMMContext(torch, sysm.n, precision, Oracle(*sysm.params(), version=1))
    stream = _stream(torch)
    for attempt in range(8):
        keep = ctx.run(k, [sysm.pos], expect=False)[0]
        if k.finish(stream) == 0:
            break
        assert list(k.withheld()) == [0] and ctx.untouched()
    else:
        raise AssertionError("the capacity negotiation did not converge in 8 attempts")
    ctx.check(*ctx.expected([sysm.pos]), 1, f"execute_openmm on variant {variant} ({precision}), the evaluation that settled")
    assert int(k.scalar("variant")) == variant
    geoms = [sysm.pos + np.random.default_rng(101 + i).normal(0.0, 0.001, sysm.pos.shape) for i in range(2)]
    keep, we, wf = ctx.run(k, geoms)
    assert k.finish(stream) == 0, (list(k.withheld()), int(k.scalar("overflow_kinds")))
    ctx.check(we, wf, 2, f"execute_openmm on variant {variant} ({precision}), two jittered evaluations")
    assert int(k.scalar("variant")) == variant
    assert int(k.scalar("launches")) == 5


@pytest.mark.parametrize("captured", ["openmm", "device"])
def test_mixing_entry_points_around_a_captured_graph_is_signalled(gpu_required, systems, five, captured):
    """The words beside the work-slot rows hold the roots' SLOTS for an evaluation that comes through execute_openmm and atom indices
    for execute_device; they are rewritten for whichever entry point enqueued last.  A graph captured through one entry has frozen
    the kernel that reads them its way, so ONE eager call through the other entry makes it stale (it would read slots as atom
    indices or the reverse; both are below n, nothing faults; with a shuffled order the roots sit at wrong positions).
    agbnp_hip_generation() is the caller's only signal: it must have changed BEFORE anything is replayed.  The caller re-captures;
    eager calls through the SAME entry between replays leave the generation alone.  (No stale graph is ever replayed here.)"""
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    k = _kernel(s)
    oracle = Oracle(*s.params(), version=1)
    ctx = OpenMMContext(torch, s.n, "double", oracle)
    assert (ctx.order != np.arange(s.n)).any()  # (slot == index would hide the defect)
    buf = _DeviceBuffers(torch, s.n)

    def eager_openmm(step, what):
        keep, we, wf = ctx.run(k, [s.jittered(step)])
        assert k.finish(_stream(torch)) == 0
        ctx.check(we, wf, 1, what)

    def eager_device(step, what):
        buf.load(s.jittered(step))
        buf.clear()
        buf.enqueue(k)
        assert k.finish(_stream(torch)) == 0
        e, f = buf.result()
        _close(what, e, f, *oracle.execute(s.jittered(step)))

    def capture():
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            (ctx if captured == "openmm" else buf).clear()
            (ctx if captured == "openmm" else buf).enqueue(k)
        return g, k.generation()

    def replay(g, step, what):
        geom = s.jittered(step)
        if captured == "openmm":
            seen = ctx.load(geom)
            g.replay()
            ctx.check(*oracle.execute(seen), 1, what)
        else:
            buf.load(geom)
            g.replay()
            e, f = buf.result()
            _close(what, e, f, *oracle.execute(geom))

    same, other = (eager_openmm, eager_device) if captured == "openmm" else (eager_device, eager_openmm)
    for step in range(3):  # warm-up outside the capture, through the entry that is captured
        same(step, f"warm-up {step}")
    g, gen = capture()
    replay(g, 5, f"graph of {captured}, replay 0")
    replay(g, 6, f"graph of {captured}, replay 1")
    other(20, "one eager evaluation through the other entry")
    assert k.generation() != gen, "an eager call through the other entry point left a captured graph stale without a signal"
    g, gen = capture()  # (what a caller does on a stale generation)
    replay(g, 7, f"second graph of {captured}, replay 0")
    replay(g, 8, f"second graph of {captured}, replay 1")
    for step in (9, 10):  # eager calls through the SAME entry between replays: the graph stays good, and the generation says so
        same(20 + step, "an eager evaluation through the same entry")
        assert k.generation() == gen
        replay(g, step, f"second graph of {captured}, replay after a same-entry eager call")
    assert k.finish(_stream(torch)) == 0
    assert k.generation() == gen


def test_a_long_step_and_a_reorder_are_withheld_once_and_repeat_right(gpu_required, systems, five):
    """The sequence that tests/test_openmm_glue.py replays through the glue (tests/golden/protocol_steps.dat), here through
    execute_openmm itself, fixture264 in double: from the settled geometry a step that moves one heavy atom by 0.1 nm (beyond the
    0.04 nm of INTEGRATION.md s.2 item 10): finish() == 1, the withheld evaluation is that one, nothing has arrived in the buffers,
    the repeat is the oracle's; a small step; a reorder of the context's atoms with a small step: withheld once, the repeat right.
    So a glue that stops repeating returns a context WITHOUT the AGBNP term for exactly these evaluations."""
    torch = pytest.importorskip("torch")
    s = systems("fixture264")
    k = _kernel(s)
    ctx = OpenMMContext(torch, s.n, "double", Oracle(*s.params(), version=1))
    stream = _stream(torch)
    geoms, moved = protocol_geometries(s.pos)
    assert len(geoms) == 4
    (atom, step), = moved[1]
    assert s.ishydrogen[atom] == 0 and 0.1 < np.linalg.norm(step) < 0.11
    assert all(np.linalg.norm(d) < 0.004 for stage in moved[2:] for _, d in stage)
    for attempt in range(8):  # settle (this fixture's largest subtree is beyond the smallest store)
        keep = ctx.run(k, [geoms[0]], expect=False)[0]
        if k.finish(stream) == 0:
            break
    else:
        raise AssertionError("the capacity negotiation did not converge in 8 attempts")
    ctx.check(*ctx.expected([geoms[0]]), 1, "settled")
    # the long step
    keep = ctx.run(k, [geoms[1]], expect=False)[0]
    assert k.finish(stream) == 1 and list(k.withheld()) == [0]
    assert int(k.scalar("overflow_kinds")) & 16
    assert ctx.untouched()
    keep, we, wf = ctx.run(k, [geoms[1]])
    assert k.finish(stream) == 0, (list(k.withheld()), int(k.scalar("overflow_kinds")))
    ctx.check(we, wf, 1, "the repeat of the long step")
    # a small step
    keep, we, wf = ctx.run(k, [geoms[2]])
    assert k.finish(stream) == 0
    ctx.check(we, wf, 1, "a small step")
    # OpenMM's reorderAtoms(), then a small step
    ctx.reorder()
    keep = ctx.run(k, [geoms[3]], expect=False)[0]
    assert k.finish(stream) == 1 and list(k.withheld()) == [0]
    assert ctx.untouched()
    keep, we, wf = ctx.run(k, [geoms[3]])
    assert k.finish(stream) == 0, (list(k.withheld()), int(k.scalar("overflow_kinds")))
    ctx.check(we, wf, 1, "the repeat after a reorder")
    assert int(k.scalar("launches")) == 5


FAMILIES = ("execute_openmm", "energy_openmm", "execute_device", "energy_device", "execute", "energy", "execute_group", "energy_group",
            "execute_group_host", "energy_group_host")
# every family once in order, once more in another order, the first one a third time: each follows two different others
EVERY_FAMILY_IN_TURN = FAMILIES + ("execute_device", "execute_openmm", "energy_group", "energy_openmm", "energy_group_host", "energy_device",
                                   "execute_group", "energy", "execute_group_host", "execute", "execute_openmm")


def test_every_entry_family_in_turn_leaves_nothing_behind(gpu_required, systems, five):
    """What a caller asks of one evaluation -- positions, targets, energy-only, the buffer to clear first, an OpenMM context's posq
    and planes -- must reach that evaluation's launches and no later one's.  trpcage, version 1, three contexts, the first of them
    also behind an OpenMM context's buffers (mixed precision): the ten entry families in an irregular order in which each follows
    at least two different others, the single-context ones on the first context, the group ones on all three, every step at fresh
    positions.  Every result is the oracle's (TIGHT for the FP64 targets; FIXED_POINT per evaluation for the planes, through
    OpenMMContext.check); an energy-only step leaves the caller's force buffer, or the planes, as loaded; nothing is withheld."""
    torch = pytest.importorskip("torch")
    sentinel, plane_sentinel = -1234.5678, 7
    followed = {name: {a for a, b in zip(EVERY_FAMILY_IN_TURN, EVERY_FAMILY_IN_TURN[1:]) if b == name} for name in FAMILIES}
    assert all(EVERY_FAMILY_IN_TURN.count(name) >= 2 and len(followed[name]) >= 2 for name in FAMILIES), followed
    s = systems("trpcage")
    assert s.n == 272
    oracle = Oracle(*s.params(), version=1)
    ks = [_kernel(s) for _ in range(3)]
    ctx = OpenMMContext(torch, s.n, "mixed", oracle)
    bufs = [Buffers(torch, s.n) for _ in ks]
    stream = _stream(torch)
    for step, what in enumerate(EVERY_FAMILY_IN_TURN):
        group, energy_only = "group" in what, what.startswith("energy")
        members = ks if group else ks[:1]
        geoms = [s.jittered(step if m == 0 else 100 * m + step) for m in range(len(members))]
        if "openmm" in what:
            hi, lo, seen = ctx.host_arrays(geoms[0])
            geoms = [seen]
            posq, corr = torch.tensor(hi, device=ctx.dev), torch.tensor(lo, device=ctx.dev)
            if energy_only:
                ctx.fixed.fill_(plane_sentinel)
        for b, g in zip(bufs, geoms):
            b.load(g, sentinel if energy_only else 0.0)
        torch.cuda.synchronize()
        want = [oracle.execute(g) for g in geoms]
        got = None  # (energy, forces or None) per member, for the families that return or accumulate FP64
        if what == "execute_openmm":
            ctx.enqueue(ks[0], posq, corr, stream)
        elif what == "energy_openmm":
            ks[0].energy_openmm(posq.data_ptr(), False, corr.data_ptr(), ctx.index.data_ptr(), ctx.padded, ctx.ebuf.data_ptr(), True,
                                ENERGY_SLOT, stream)
        elif what == "execute_device":
            ks[0].execute_device(*bufs[0].ptrs(), stream)
        elif what == "energy_device":
            ks[0].energy_device(bufs[0].pos.data_ptr(), bufs[0].ene.data_ptr(), stream)
        elif what == "execute":
            f = np.zeros((s.n, 3))
            got = [(ks[0].execute(geoms[0], f), f)]
        elif what == "energy":
            got = [(ks[0].energy(geoms[0]), None)]
        elif what == "execute_group":
            execute_group(ks, bufs, stream)
        elif what == "energy_group":
            P.energy_group(ks, [b.pos.data_ptr() for b in bufs], [b.ene.data_ptr() for b in bufs], stream)
        elif what == "execute_group_host":
            fs = [np.zeros((s.n, 3)) for _ in ks]
            got = list(zip(P.execute_group_host(ks, geoms, fs), fs))
        else:
            got = [(e, None) for e in P.energy_group_host(ks, geoms)]
        assert [k.finish(stream) for k in members] == [0] * len(members), (step, what)
        if what == "execute_openmm":
            ctx.check(*want[0], 1, f"step {step}, {what}")
            continue
        if what == "energy_openmm":
            assert (ctx.fixed == plane_sentinel).all(), "an energy-only evaluation wrote to the fixed-point planes"
            de = abs(ctx.energy() - want[0][0])
            print(f"step {step}, {what}: |dE|={de:.3e}")
            energy_close(ctx.energy(), want[0][0])
            ctx.clear()
            continue
        if got is None:
            got = [b.result() for b in bufs[: len(members)]]
            if energy_only:
                assert all((f == sentinel).all() for _, f in got), "an energy-only evaluation wrote to a caller's force buffer"
                got = [(e, None) for e, _ in got]
        for m, ((e, f), (eo, fo)) in enumerate(zip(got, want)):
            df = 0.0 if f is None else np.abs(f - fo).max()
            print(f"step {step}, {what}, member {m}: |dE|={abs(e - eo):.3e}  max|dF|={df:.3e}")
            if f is None:
                energy_close(e, eo)
            else:
                close(e, f, eo, fo)
