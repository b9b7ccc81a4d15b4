"""GPU box: the cavity launch's single-gather form (csrc/tree_bodies.h, cavity_forests SINGLE).  An evaluation that
ends in a pseudo-volume replay walks a forest's membership list ONCE in the cavity launch -- gradient of the enlarged-radius pass,
self volumes of the vdW pass -- and the replay carries the vdW-radius cavity gradient with per-atom weights nu - gamma/roffset.
Every entry family that shares those bodies against the CPU oracle (ReferenceAGBNPKernels.cpp:293-384, 718-747) at the tolerance of
tests/test_gpu_healing.py; version 0, which has no replay, keeps both gathers."""
import numpy as np
import pytest

import openmm_agbnp_plugin_amd as P
from oracle import Oracle
from tests.gpu_helpers import SAME, TIGHT, Buffers, close, execute_group, freeze_packing, kernel_of
from tests.gpu_helpers import five_groups  # noqa: F401
from tests.openmm_context import OpenMMContext

pytestmark = pytest.mark.gpu


def _check(what, e, f, eo, fo, evaluations=1):
    """Energy and forces against the oracle's sums over `evaluations` accumulated evaluations: TIGHT each; figures first."""
    de, df = abs(e - eo), float(np.abs(f - fo).max())
    print(f"{what}: {evaluations} evaluation(s)  |dE|={de:.3e}  max|dF|={df:.3e}")
    assert de < evaluations * TIGHT, f"{what}: energy differs by {de:.3e}"
    assert df < evaluations * TIGHT, f"{what}: forces differ by {df:.3e}"


def _queue(k, torch, geoms, n):
    dev = torch.device("cuda:0")
    pos = torch.tensor(np.stack(geoms), dtype=torch.float64, device=dev).contiguous()
    frc = torch.zeros((n, 3), dtype=torch.float64, device=dev)
    ene = torch.zeros((1,), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    run = lambda i: k.execute_device(pos[i].data_ptr(), frc.data_ptr(), ene.data_ptr(), stream)
    return run, frc, ene, stream


def _scaled_gammas(s, seed=3):
    """Non-uniform per-atom gammas: each scaled by 0.5 .. 1.5."""
    return np.asarray(s.gamma) * np.random.default_rng(seed).uniform(0.5, 1.5, s.n)


def _with_gammas(s, gamma, version=1):
    return P.AGBNPForce.from_arrays(s.radius, gamma, s.alpha, s.charge, s.ishydrogen, version=version)


@pytest.mark.parametrize("launches", ["five", "six"])
def test_queued_geometries_in_both_launch_chains(gpu_required, systems, monkeypatch, launches):
    """trpcage, version 1: three jittered geometries queued through execute_device, each on buffers of its own sum."""
    torch = pytest.importorskip("torch")
    monkeypatch.setenv("AGBNP_HIP_FIVE_LAUNCHES", "1" if launches == "five" else "0")
    s = systems("trpcage")
    oracle = Oracle(*s.params(), version=1)
    k = kernel_of(s.params())
    geoms = [s.jittered(step) for step in range(3)]
    run, frc, ene, stream = _queue(k, torch, geoms, s.n)
    for i in (0, 1):  # settle on the engine's own packing
        run(i)
    assert k.finish(stream) == 0
    assert int(k.scalar("launches")) == (5 if launches == "five" else 6)
    for i, g in enumerate(geoms):
        frc.zero_()
        ene.zero_()
        run(i)
        assert k.finish(stream) == 0
        _check(f"{launches}-launch chain, geometry {i}", ene.item(), frc.cpu().numpy(), *oracle.execute(g))


@pytest.mark.parametrize("gammas", ["scaled", "zero"])
def test_changed_gammas_reach_both_tree_launches(gpu_required, systems, five_groups, gammas):
    """update_parameters between two evaluations: the replay reads the context's gamma row, so the next evaluation must be the
    oracle's with the new gammas.  All gammas zero: the cavity part vanishes from both tree launches.  (Per-atom gammas exist
    behind an update only -- creation refuses them, in the reference, the oracle and the engine alike -- so the oracle gets
    them the same way: ReferenceAGBNPKernels.cpp copyParametersToContext, oracle.update.)"""
    s = systems("trpcage")
    k = kernel_of(s.params())
    oracle = Oracle(*s.params(), version=1)
    f = np.zeros((s.n, 3))
    e = k.execute(s.pos, f)
    _check("before the update", e, f, *oracle.execute(s.pos))
    new = _scaled_gammas(s) if gammas == "scaled" else np.zeros(s.n)
    k.copyParametersToContext(_with_gammas(s, new))
    oracle.update(s.radius, new, s.alpha, s.charge, s.ishydrogen)
    for step in (0, 1):
        pos = s.jittered(step, sigma=0.004)
        f = np.zeros((s.n, 3))
        e = k.execute(pos, f)
        _check(f"gammas {gammas}, evaluation {step} after the update", e, f, *oracle.execute(pos))


def test_healed_sets_carry_the_combined_weight(gpu_required, systems, five_groups):
    """1dwc with the packing frozen at eight whole subtrees per forest: every forest is rebuilt in smaller sets, the later ones
    replayed from spare slots.  Two geometries: nothing withheld, the oracle's sums."""
    torch = pytest.importorskip("torch")
    s = systems("1dwc")
    oracle = Oracle(*s.params(), version=1)
    k = kernel_of(s.params())
    geoms = [s.jittered(step) for step in range(2)]
    run, frc, ene, stream = _queue(k, torch, geoms, s.n)
    for i in (0, 1):
        run(i)
    assert k.finish(stream) == 0
    freeze_packing(k, s.nheavy)
    frc.zero_()
    ene.zero_()
    for i in (0, 1):
        run(i)
    assert k.finish(stream) == 0, (list(k.withheld()), int(k.scalar("overflow_kinds")))
    assert int(k.scalar("healed_forests")) > 0
    want = [oracle.execute(g) for g in geoms]
    _check("healed forests", ene.item(), frc.cpu().numpy(), want[0][0] + want[1][0], want[0][1] + want[1][1], 2)


def test_version_0_keeps_both_gathers(gpu_required, systems, five_groups):
    """No replay to carry anything: two launches, the oracle's energy and forces."""
    s = systems("trpcage")
    k = kernel_of(s.params(), version=0)
    oracle = Oracle(*s.params(), version=0)
    for step in (0, 1):
        pos = s.jittered(step, sigma=0.004)
        f = np.zeros((s.n, 3))
        e = k.execute(pos, f)
        _check(f"version 0, evaluation {step}", e, f, *oracle.execute(pos))
    assert int(k.scalar("launches")) == 2


@pytest.mark.parametrize("precision", ["double", "mixed"])
def test_the_openmm_entry_in_a_shuffled_order(gpu_required, systems, five_groups, precision):
    """The POSQ instantiations: posq in a shuffled, padded context order, forces into the fixed-point planes."""
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    k = kernel_of(s.params())
    oracle = Oracle(*s.params(), version=1)
    ctx = OpenMMContext(torch, s.n, precision, oracle)
    stream = torch.cuda.current_stream().cuda_stream
    keep = ctx.run(k, [s.jittered(0), s.jittered(1)], expect=False)[0]  # settle
    assert k.finish(stream) == 0
    ctx.clear()
    keep, we, wf = ctx.run(k, [s.jittered(2)])
    assert k.finish(stream) == 0
    _check(f"execute_openmm ({precision})", ctx.energy(), ctx.forces(), we, wf)
    assert int(k.scalar("launches")) == 5 and keep


def test_a_captured_graph_replays_on_new_geometries(gpu_required, systems, five_groups):
    """The DEVPAR instantiations (the device names the evaluation's set): one execute_device captured, replayed on two geometries."""
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    k = kernel_of(s.params())
    oracle = Oracle(*s.params(), version=1)
    buf = Buffers(torch, s.n)
    stream = torch.cuda.current_stream().cuda_stream
    for step in (0, 1):  # settle, outside the capture
        buf.load(s.jittered(step))
        k.execute_device(*buf.ptrs(), stream)
    assert k.finish(stream) == 0
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        buf.frc.zero_()
        buf.ene.zero_()
        k.execute_device(*buf.ptrs(), torch.cuda.current_stream().cuda_stream)
    for step in (2, 3):
        geom = s.jittered(step)
        buf.pos.copy_(torch.tensor(geom, dtype=torch.float64))
        g.replay()
        torch.cuda.synchronize()
        _check(f"captured graph, replay {step - 2}", *buf.result(), *oracle.execute(geom))
    assert k.finish(stream) == 0


def test_a_replica_group_with_different_gammas(gpu_required, systems, five_groups):
    """k_group_cavity_five and the group replay: two trpcage contexts, each with gammas of its own -- the file's, and per-atom
    ones given by an update -- against its own oracle."""
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    ks = [kernel_of(s.params()) for _ in range(2)]
    oracles = [Oracle(*s.params(), version=1) for _ in range(2)]
    new = _scaled_gammas(s, seed=9)
    ks[1].copyParametersToContext(_with_gammas(s, new))
    oracles[1].update(s.radius, new, s.alpha, s.charge, s.ishydrogen)
    stream = torch.cuda.current_stream().cuda_stream
    bufs = [Buffers(torch, s.n) for _ in ks]
    for step in range(3):
        geoms = [s.jittered(10 * m + step) for m in range(2)]
        for b, g in zip(bufs, geoms):
            b.load(g)
        execute_group(ks, bufs, stream)
        assert [k.finish(stream) for k in ks] == [0, 0]
        for m in range(2):
            _check(f"group member {m}, step {step}", *bufs[m].result(), *oracles[m].execute(geoms[m]))
    assert [int(k.scalar("group_members")) for k in ks] == [2, 2]


def test_an_energy_only_evaluation_between_two_full_ones(gpu_required, systems, five_groups):
    """The energy-only evaluation runs the cavity launch in the same form and no replay: it must leave the context as a full
    evaluation does, and its energy is the full evaluation's."""
    s = systems("trpcage")
    k = kernel_of(s.params())
    oracle = Oracle(*s.params(), version=1)
    pos = [s.jittered(step, sigma=0.004) for step in range(3)]
    f = np.zeros((s.n, 3))
    e = k.execute(pos[0], f)
    _check("full evaluation before", e, f, *oracle.execute(pos[0]))
    e_only = k.energy(pos[1])
    f = np.zeros((s.n, 3))
    e_full = k.execute(pos[1], f)
    print(f"energy-only against full: {abs(e_only - e_full):.3e}")
    assert abs(e_only - e_full) < SAME
    _check("full evaluation at the energy-only geometry", e_full, f, *oracle.execute(pos[1]))
    f = np.zeros((s.n, 3))
    e = k.execute(pos[2], f)
    _check("full evaluation after", e, f, *oracle.execute(pos[2]))
    assert int(k.scalar("energy_only_launches")) == 4


def test_deterministic_mode_stays_bitwise_reproducible(gpu_required, systems):
    """The quantised terms of the replay are those of the combined weight: the bits may differ from earlier libraries', not from
    run to run.  Two fresh contexts, the geometries in different sequences; the oracle at the tolerance of
    tests/test_gpu_parity.py::test_deterministic_mode_is_bit_reproducible (assert_close: 1e-7)."""
    s = systems("trpcage")
    geoms = [s.pos, s.jittered(1, sigma=0.004)]

    def run(order):
        k = kernel_of(s.params(), mode="deterministic")
        out = {}
        for g in order:
            f = np.zeros((s.n, 3))
            out[g] = (k.execute(geoms[g], f), f)
        return out

    a, b = run([0, 1, 0]), run([1, 1, 0])
    oracle = Oracle(*s.params(), version=1)
    for g in range(2):
        assert a[g][0] == b[g][0], f"energy of geometry {g} differs between two runs"
        assert np.array_equal(a[g][1], b[g][1]), f"forces of geometry {g} differ by {np.abs(a[g][1] - b[g][1]).max():.3e}"
        eo, fo = oracle.execute(geoms[g])
        de, df = abs(a[g][0] - eo), float(np.abs(a[g][1] - fo).max())
        print(f"deterministic mode, geometry {g}: |dE|={de:.3e}  max|dF|={df:.3e}")
        close(a[g][0], a[g][1], eo, fo)
