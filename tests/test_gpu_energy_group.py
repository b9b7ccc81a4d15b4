"""GPU box: energy-only replica groups and the jump hint (include/agbnp_hip.h: agbnp_hip_energy_group / _host,
agbnp_hip_expect_jump).  Every member of an energy group must get what its own agbnp_hip_energy_device would
give it -- the oracle's energy, the energy of a twin context evaluated alone, its own overflow log, no force written anywhere --
and be left as a full evaluation leaves it.  A hinted evaluation at unrelated positions is complete at the first try."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import openmm_agbnp_plugin_amd as P
from openmm_agbnp_plugin_amd import _lib
from oracle import Oracle
from tests.gpu_helpers import SAME, TIGHT, Buffers
from tests.gpu_helpers import cluster as _cluster
from tests.gpu_helpers import execute_group as _fgroup
from tests.gpu_helpers import five_groups as five  # noqa: F401
from tests.gpu_helpers import kernel_of as _kernel

pytestmark = pytest.mark.gpu
SENTINEL = -1234.5678
JUMP = 16  # scalar 15: the evaluation was void because heavy atoms had left the neighbour masks' skin


def _energy_close(e, eo, tol=TIGHT):
    print(f"energy {e!r} reference {eo!r} difference {abs(e - eo):.3e}")
    assert abs(e - eo) < tol * max(1.0, abs(eo) * 1e-3), f"energy differs by {abs(e - eo):.3e}"


def _close(e, f, eo, fo, tol=TIGHT):
    _energy_close(e, eo, tol)
    print(f"forces differ by {np.abs(f - fo).max():.3e}")
    assert np.abs(f - fo).max() < tol, f"forces differ by {np.abs(f - fo).max():.3e}"


def _egroup(kernels, bufs, stream):
    P.energy_group(kernels, [b.pos.data_ptr() for b in bufs], [b.ene.data_ptr() for b in bufs], stream)


def _kinds(ks):
    return [int(k.scalar("last_evaluation_kind")) for k in ks]


def _members(ks):
    return [int(k.scalar("group_members")) for k in ks]


@pytest.mark.parametrize("version,name", [(1, "trpcage"), (1, "1dwc"), (1, "fixture264"), (0, "trpcage")])
@pytest.mark.parametrize("R", [1, 2, 4])
def test_energy_group_matches_the_oracle_and_twins_alone(gpu_required, systems, five, version, name, R):
    """R contexts of one system, each on a jittered trajectory of its own: every member's energy is the oracle's and that of a
    twin context evaluated alone through energy_device; the members share one launch set of energy-only launches."""
    torch = pytest.importorskip("torch")
    s = systems(name)
    oracle = Oracle(*s.params(), version=version)
    ks = [_kernel(s.params(), version) for _ in range(R)]
    twins = [_kernel(s.params(), version) for _ in range(R)]
    stream = torch.cuda.current_stream().cuda_stream
    bufs = [Buffers(torch, s.n) for _ in range(R)]
    tb = [Buffers(torch, s.n) for _ in range(R)]
    for step in range(6):
        geoms = [s.jittered(100 * m + step) for m in range(R)]
        for b, t, g in zip(bufs, tb, geoms):
            b.load(g, SENTINEL)
            t.load(g)
        _egroup(ks, bufs, stream)
        for tw, t in zip(twins, tb):
            tw.energy_device(t.pos.data_ptr(), t.ene.data_ptr(), stream)
        for m in range(R):
            withheld = ks[m].finish(stream)
            assert twins[m].finish(stream) == withheld
            if withheld:  # (a capacity climb: repeated through the group, as a caller of energy_device repeats)
                assert bufs[m].result()[0] == 0.0
                bufs[m].load(geoms[m], SENTINEL)
                _egroup([ks[m]], [bufs[m]], stream)
                assert ks[m].finish(stream) == 0
                tb[m].load(geoms[m])
                twins[m].energy_device(tb[m].pos.data_ptr(), tb[m].ene.data_ptr(), stream)
                assert twins[m].finish(stream) == 0
            e, f = bufs[m].result()
            assert (f == SENTINEL).all()
            _energy_close(e, oracle.execute(geoms[m])[0])
            _energy_close(e, tb[m].result()[0], tol=SAME)
        if all(int(k.scalar("variant")) <= 3 for k in ks):
            assert _members(ks) == [R] * R
            assert _kinds(ks) == [1] * R


def test_no_force_is_written_and_the_state_is_a_full_evaluations(gpu_required, systems, five):
    """Energy groups and full groups alternate on the same three contexts so that both kinds meet both parities of the
    five-launch mode's sets.  An energy call leaves the force buffers' sentinel alone; every full result equals the oracle's and
    that of a twin that only ever ran full evaluations; after the first four calls no argument block is rewritten any more."""
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    oracle = Oracle(*s.params(), version=1)
    ks = [_kernel(s.params()) for _ in range(3)]
    twins = [_kernel(s.params()) for _ in range(3)]
    stream = torch.cuda.current_stream().cuda_stream
    bufs = [Buffers(torch, s.n) for _ in ks]
    tb = [Buffers(torch, s.n) for _ in ks]
    settled = None
    for step, what in enumerate("FEEFFEEFEF"):
        geoms = [s.jittered(40 * m + step) for m in range(3)]
        for b, t, g in zip(bufs, tb, geoms):
            b.load(g, SENTINEL if what == "E" else 0.0)
            t.load(g)
        (_egroup if what == "E" else _fgroup)(ks, bufs, stream)
        for tw, t in zip(twins, tb):
            tw.execute_device(*t.ptrs(), stream)
        assert [k.finish(stream) for k in ks] == [0, 0, 0]
        assert [k.finish(stream) for k in twins] == [0, 0, 0]
        assert _kinds(ks) == [1 if what == "E" else 0] * 3
        assert _members(ks) == [3, 3, 3]
        for b, t, g in zip(bufs, tb, geoms):
            e, f = b.result()
            eo, fo = oracle.execute(g)
            if what == "E":
                assert (f == SENTINEL).all(), "an energy-only group call wrote to a force buffer"
                _energy_close(e, eo)
                _energy_close(e, t.result()[0], tol=SAME)
            else:
                _close(e, f, eo, fo)
                _close(e, f, *t.result(), tol=SAME)
        writes = [int(k.scalar("group_block_writes")) for k in ks]
        print(step, what, "group_block_writes", writes)
        if step == 3:
            settled = writes
        if step > 3:
            assert writes == settled, "a steady run of mixed group calls rewrote an argument block"
    assert settled == [2, 2, 2]  # (one write per parity, whichever kind of call met it first)


def test_heterogeneous_members(gpu_required, systems, five):
    """trpcage, 1dwc and 2clr (version 1), a version-0 trpcage and a trpcage with its charges halved in one call: each matches its
    own oracle; the version-0 member is a launch set of its own."""
    torch = pytest.importorskip("torch")
    tp, d1, c2 = systems("trpcage"), systems("1dwc"), systems("2clr")
    half = list(tp.params())
    half[3] = np.asarray(half[3]) * 0.5
    members = [(tp, tp.params(), 1), (d1, d1.params(), 1), (c2, c2.params(), 1), (tp, tp.params(), 0), (tp, tuple(half), 1)]
    ks = [_kernel(prm, v) for _, prm, v in members]
    oracles = [Oracle(*prm, version=v) for _, prm, v in members]
    stream = torch.cuda.current_stream().cuda_stream
    bufs = [Buffers(torch, s.n) for s, _, _ in members]
    for step in range(3):
        geoms = [s.jittered(step + 7 * m) for m, (s, _, _) in enumerate(members)]
        for b, g in zip(bufs, geoms):
            b.load(g)
        _egroup(ks, bufs, stream)
        assert [k.finish(stream) for k in ks] == [0] * len(ks)
        for b, o, g in zip(bufs, oracles, geoms):
            _energy_close(b.result()[0], o.execute(g)[0])
    assert int(ks[3].scalar("group_members")) == 1
    v1 = [k for (_, _, v), k in zip(members, ks) if v == 1]
    for k in v1:
        same = sum(1 for j in v1 if int(j.scalar("variant")) == int(k.scalar("variant")))
        assert int(k.scalar("group_members")) == same
    assert _kinds(ks) == [1] * len(ks)


def test_members_that_cannot_share_run_alone(gpu_required, systems, five, monkeypatch):
    """A deterministic-mode member and a member with diagnostics run as full evaluations with their forces sent to a buffer of
    their own (scalar 19 = 0, scalar 20 = 2) and are right; the two others share energy-only launches.  With
    AGBNP_HIP_GROUP_LAUNCHES=0 everyone runs alone -- the members that can on their own energy-only launches (kind 1) -- with the
    same numbers."""
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    oracle = Oracle(*s.params(), version=1)
    stream = torch.cuda.current_stream().cuda_stream

    def run(expect_members, expect_kinds):
        ks = [_kernel(s.params()), _kernel(s.params(), mode="deterministic"), _kernel(s.params()), _kernel(s.params())]
        _lib.load().agbnp_hip_set_diagnostics(ks[2]._h, 1)
        bufs = [Buffers(torch, s.n) for _ in ks]
        energies = []
        for step in range(3):
            geoms = [s.jittered(step + 11 * m) for m in range(len(ks))]
            for b, g in zip(bufs, geoms):
                b.load(g, SENTINEL)
            _egroup(ks, bufs, stream)
            assert [k.finish(stream) for k in ks] == [0] * len(ks)
            for b, g in zip(bufs, geoms):
                e, f = b.result()
                assert (f == SENTINEL).all()
                _energy_close(e, oracle.execute(g)[0])
                energies.append(e)
        assert _members(ks) == expect_members
        assert _kinds(ks) == expect_kinds
        return energies

    shared = run([2, 0, 0, 2], [1, 2, 2, 1])
    monkeypatch.setenv("AGBNP_HIP_GROUP_LAUNCHES", "0")
    alone = run([0, 0, 0, 0], [1, 2, 2, 1])
    for a, b in zip(shared, alone):
        _energy_close(a, b, tol=SAME)
    ks = [_kernel(s.params()) for _ in range(2)]  # (ordinary members only: everyone alone, everyone kind 1)
    bufs = [Buffers(torch, s.n) for _ in ks]
    for b, m in zip(bufs, range(2)):
        b.load(s.jittered(m))
    _egroup(ks, bufs, stream)
    assert [k.finish(stream) for k in ks] == [0, 0]
    assert _members(ks) == [0, 0] and _kinds(ks) == [1, 1]
    for b, m in zip(bufs, range(2)):
        _energy_close(b.result()[0], oracle.execute(s.jittered(m))[0])


def test_a_jump_is_withheld_for_that_member_only(gpu_required, systems, five):
    """One member jumps 0.1 nm: only its finish() reports a withheld evaluation and its energy word received nothing; the others
    are complete and right.  Its repeat, through an energy group of one and through energy_device, is right."""
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    oracle = Oracle(*s.params(), version=1)
    ks = [_kernel(s.params()) for _ in range(3)]
    stream = torch.cuda.current_stream().cuda_stream
    bufs = [Buffers(torch, s.n) for _ in ks]
    geoms = [s.jittered(m) for m in range(3)]
    for b, g in zip(bufs, geoms):
        b.load(g)
    _egroup(ks, bufs, stream)
    assert [k.finish(stream) for k in ks] == [0, 0, 0]
    geoms = [s.jittered(10 + m) for m in range(3)]
    geoms[1] = geoms[1] + np.array([0.1, 0.0, 0.0])
    for b, g in zip(bufs, geoms):
        b.load(g)
    _egroup(ks, bufs, stream)
    assert [k.finish(stream) for k in ks] == [0, 1, 0]
    assert list(ks[1].withheld()) == [0]
    assert int(ks[1].scalar("overflow_kinds")) & JUMP
    assert bufs[1].result()[0] == 0.0
    for m in (0, 2):
        _energy_close(bufs[m].result()[0], oracle.execute(geoms[m])[0])
    bufs[1].load(geoms[1])
    _egroup([ks[1]], [bufs[1]], stream)  # the repeat through a group ...
    assert ks[1].finish(stream) == 0
    _energy_close(bufs[1].result()[0], oracle.execute(geoms[1])[0])
    jump = geoms[1] - np.array([0.1, 0.0, 0.0])
    bufs[1].load(jump)
    _egroup(ks[1:2], bufs[1:2], stream)
    assert ks[1].finish(stream) == 1
    assert bufs[1].result()[0] == 0.0
    bufs[1].load(jump)
    ks[1].energy_device(bufs[1].pos.data_ptr(), bufs[1].ene.data_ptr(), stream)  # ... and through a single call
    assert ks[1].finish(stream) == 0
    _energy_close(bufs[1].result()[0], oracle.execute(jump)[0])


def _scaled_charges(params, scale):
    prm = list(params)
    prm[3] = np.asarray(prm[3]) * scale
    return tuple(prm)


def test_the_hint_makes_cross_evaluations_complete(gpu_required, systems, five, monkeypatch):
    """An exchange matrix U_i(x_j) over three Hamiltonians (charges scaled 1, 0.5, 0) and three unrelated conformations, one
    energy group per cyclic shift with expect_jump() on every member in front: no evaluation is withheld for a jump and every
    entry is the oracle's.  Without the hint the same kind of evaluation is withheld as a jump.  The hint works in front of the
    single-context entry points as well and does nothing on the six-launch path."""
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    params = [_scaled_charges(s.params(), q) for q in (1.0, 0.5, 0.0)]
    oracles = [Oracle(*prm, version=1) for prm in params]
    ks = [_kernel(prm) for prm in params]
    xs = [s.jittered(1000 + m, sigma=0.02) for m in (1, 2, 3)]
    heavy = np.asarray(s.params()[4]) == 0
    for a in range(3):
        for b in range(a):  # (what makes them unrelated: most heavy atoms are beyond the 0.04 nm a context tolerates)
            d = np.linalg.norm(xs[a] - xs[b], axis=1)[heavy]
            print(f"conformations {a} {b}: {np.mean(d > 0.04):.2f} of the heavy atoms beyond 0.04 nm, largest move {d.max():.3f} nm")
            assert np.mean(d > 0.04) >= 0.5
    stream = torch.cuda.current_stream().cuda_stream
    dev = torch.device("cuda:0")
    xbuf = [torch.tensor(x, dtype=torch.float64, device=dev) for x in xs]  # one buffer per conformation, shared between members
    ene = torch.zeros(3, dtype=torch.float64, device=dev)  # a contiguous array, one word per member
    for p in range(3):
        at = [(i + p) % 3 for i in range(3)]
        ene.zero_()
        for k in ks:
            k.expect_jump()
        P.energy_group(ks, [xbuf[j].data_ptr() for j in at], [ene.data_ptr() + 8 * i for i in range(3)], stream)
        for i, k in enumerate(ks):
            if k.finish(stream):  # (not a jump: a caller repeats it once)
                kinds = int(k.scalar("overflow_kinds"))
                print(f"shift {p} member {i}: withheld, kinds {kinds}")
                assert not kinds & JUMP, "a hinted evaluation was withheld as a jump"
                assert ene[i].item() == 0.0
                P.energy_group([k], [xbuf[at[i]].data_ptr()], [ene.data_ptr() + 8 * i], stream)
                assert k.finish(stream) == 0
            _energy_close(ene[i].item(), oracles[i].execute(xs[at[i]])[0])
        assert _kinds(ks) == [1, 1, 1]
    # the control: member 0 is at conformation 2 now; conformation 1 without the hint is a jump
    ene.zero_()
    P.energy_group(ks[:1], [xbuf[1].data_ptr()], [ene.data_ptr()], stream)
    assert ks[0].finish(stream) == 1
    assert int(ks[0].scalar("overflow_kinds")) & JUMP
    assert ene[0].item() == 0.0
    # (its repeat is complete: the device has laid the masks down anew in the withheld evaluation)
    P.energy_group(ks[:1], [xbuf[1].data_ptr()], [ene.data_ptr()], stream)
    assert ks[0].finish(stream) == 0
    _energy_close(ene[0].item(), oracles[0].execute(xs[1])[0])

    # the same hint in front of the single-context entry points: member 0 goes 1 -> 2 -> 0 -> 1
    k, oracle, b = ks[0], oracles[0], Buffers(torch, s.n)

    def complete(withheld):
        if withheld:
            kinds = int(k.scalar("overflow_kinds"))
            print("single-context call withheld, kinds", kinds)
            assert not kinds & JUMP, "a hinted evaluation was withheld as a jump"
        return not withheld

    b.load(xs[2])
    k.expect_jump()
    k.execute_device(*b.ptrs(), stream)
    if not complete(k.finish(stream)):
        b.load(xs[2])
        k.execute_device(*b.ptrs(), stream)
        assert k.finish(stream) == 0
    _close(*b.result(), *oracle.execute(xs[2]))
    assert _kinds([k]) == [0]
    b.load(xs[0])
    k.expect_jump()
    k.energy_device(b.pos.data_ptr(), b.ene.data_ptr(), stream)
    if not complete(k.finish(stream)):
        b.load(xs[0])
        k.energy_device(b.pos.data_ptr(), b.ene.data_ptr(), stream)
        assert k.finish(stream) == 0
    _energy_close(b.result()[0], oracle.execute(xs[0])[0])
    # execute() repeats a withheld evaluation inside: how often it ran shows in the launch counts of the profiling timeline
    k.set_profiling(True)
    k.expect_jump()
    f = np.zeros((s.n, 3))
    e = k.execute(xs[1], f)
    times = {n: v[1] for n, v in k.kernel_times().items() if v[1] > 0}
    print("hinted execute():", times)
    assert times["k_tree_cavity"] == 1 and times["k_prep"] == 1, times  # (k_prep: what the mask launch is booked as)
    _close(e, f, *oracle.execute(xs[1]))
    assert int(k.scalar("launches")) == 5
    k.set_profiling(True)  # (resets the counts) ... and without the hint execute() does repeat a jump inside
    f = np.zeros((s.n, 3))
    e = k.execute(xs[2], f)
    times = {n: v[1] for n, v in k.kernel_times().items() if v[1] > 0}
    print("execute() without the hint:", times)
    k.set_profiling(False)
    assert times["k_tree_cavity"] == 2 and "k_prep" not in times, times
    _close(e, f, *oracle.execute(xs[2]))

    # the six-launch path lays the masks down at every evaluation: the hint does nothing there
    monkeypatch.setenv("AGBNP_HIP_FIVE_LAUNCHES", "0")
    k6 = _kernel(params[0])
    for x in (xs[0], xs[1], xs[2]):
        b.load(x)
        k6.expect_jump()
        k6.execute_device(*b.ptrs(), stream)
        assert k6.finish(stream) == 0
        _close(*b.result(), *oracle.execute(x))
    b.load(xs[0])
    k6.expect_jump()
    P.energy_group([k6], [b.pos.data_ptr()], [b.ene.data_ptr()], stream)
    assert k6.finish(stream) == 0
    _energy_close(b.result()[0], oracle.execute(xs[0])[0])
    assert _kinds([k6]) == [2] and int(k6.scalar("launches")) == 6


def test_a_pending_hint_is_not_captured(gpu_required, systems, five):
    """expect_jump() in front of an evaluation that is enqueued inside a stream capture: the graph replays as it would have
    without the hint, the hint stays pending, and the next eager evaluation -- at a far conformation -- consumes it and is
    complete at the first try; the one after that, far again and not announced, is a jump."""
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    k = _kernel(s.params())
    oracle = Oracle(*s.params(), version=1)
    f0 = np.zeros((s.n, 3))
    for step in range(3):
        k.execute(s.jittered(step), f0)
    b = Buffers(torch, s.n)
    b.load(s.jittered(4))
    k.expect_jump()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        b.frc.zero_()
        b.ene.zero_()
        k.execute_device(*b.ptrs(), torch.cuda.current_stream().cuda_stream)
    for step in (5, 6):
        geom = s.jittered(step)
        b.pos.copy_(torch.tensor(geom, dtype=torch.float64))
        g.replay()
        torch.cuda.synchronize()
        _close(*b.result(), *oracle.execute(geom))
    stream = torch.cuda.current_stream().cuda_stream
    assert k.finish(stream) == 0
    far = [s.jittered(1000 + m, sigma=0.02) for m in (1, 2)]
    b.load(far[0])
    k.execute_device(*b.ptrs(), stream)  # (eager: the pending hint goes in front of this one)
    if k.finish(stream):
        kinds = int(k.scalar("overflow_kinds"))
        print("withheld, kinds", kinds)
        assert not kinds & JUMP, "the hint did not stay pending through the capture"
        b.load(far[0])
        k.execute_device(*b.ptrs(), stream)
        assert k.finish(stream) == 0
    _close(*b.result(), *oracle.execute(far[0]))
    assert int(k.scalar("launches")) == 5
    b.load(far[1])
    k.execute_device(*b.ptrs(), stream)
    assert k.finish(stream) == 1 and int(k.scalar("overflow_kinds")) & JUMP  # (consumed: this one is a jump again)


def test_energy_groups_interleave_with_everything(gpu_required, systems, five):
    """Energy groups mixed with full groups, execute_device, energy_device, execute() and energy() on the same contexts in an
    irregular order, with the NULL stream: every result is the oracle's."""
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    oracle = Oracle(*s.params(), version=1)
    ks = [_kernel(s.params()) for _ in range(3)]
    bufs = [Buffers(torch, s.n) for _ in ks]
    plan = ["egroup", "group", "egroup", "egroup", "device", "egroup", "host", "energy", "egroup", "group", "ehost", "egroup",
            "energy", "group", "egroup"]
    for step, what in enumerate(plan):
        geoms = [s.jittered(3 * step + m) for m in range(3)]
        for b, g in zip(bufs, geoms):
            b.load(g)
        torch.cuda.synchronize()
        if what == "egroup":
            _egroup(ks, bufs, None)
        if what == "group":
            _fgroup(ks, bufs, None)
        for m, k in enumerate(ks):
            eo, fo = oracle.execute(geoms[m])
            if what == "device":
                k.execute_device(*bufs[m].ptrs(), None)
            elif what == "energy":
                k.energy_device(bufs[m].pos.data_ptr(), bufs[m].ene.data_ptr(), None)
            elif what == "host":
                f = np.zeros((s.n, 3))
                _close(k.execute(geoms[m], f), f, eo, fo)
                continue
            elif what == "ehost":
                _energy_close(k.energy(geoms[m]), eo)
                continue
            assert k.finish(None) == 0
            e, f = bufs[m].result()
            if what in ("energy", "egroup"):
                assert not f.any()
                _energy_close(e, eo)
            else:
                _close(e, f, eo, fo)


def test_refusals_change_nothing(gpu_required, systems, five):
    """Inside a stream capture the call is refused and the capture still completes and replays; count 0 or 17, a NULL entry, the
    same context twice and overlapping energy words are refused; no member's enqueue index advanced, and the next energy group
    is right."""
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    oracle = Oracle(*s.params(), version=1)
    ks = [_kernel(s.params()) for _ in range(2)]
    stream = torch.cuda.current_stream().cuda_stream
    bufs = [Buffers(torch, s.n) for _ in ks]
    for b, m in zip(bufs, range(2)):
        b.load(s.jittered(m))
    _egroup(ks, bufs, stream)
    assert [k.finish(stream) for k in ks] == [0, 0]
    bufs[0].ene.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        bufs[0].ene.add_(1.0)
        with pytest.raises(P.OpenMMException):
            _egroup(ks, bufs, torch.cuda.current_stream().cuda_stream)
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    assert bufs[0].ene.item() == 2.0
    lib = _lib.load()
    hs = (C.c_void_p * 17)(*([ks[0]._h, ks[1]._h] * 9)[:17])
    vp = lambda ptrs: (C.c_void_p * len(ptrs))(*ptrs)  # noqa: E731
    pos = vp([b.pos.data_ptr() for b in bufs] * 9)
    ene = vp([bufs[0].ene.data_ptr(), bufs[1].ene.data_ptr()] + [bufs[1].ene.data_ptr()] * 16)
    assert lib.agbnp_hip_energy_group(hs, 0, pos, ene, None) == _lib.ERR_INVALID_ARGUMENT
    assert lib.agbnp_hip_energy_group(hs, 17, pos, ene, None) == _lib.ERR_INVALID_ARGUMENT
    twice = (C.c_void_p * 2)(ks[0]._h, ks[0]._h)
    assert lib.agbnp_hip_energy_group(twice, 2, pos, ene, None) == _lib.ERR_INVALID_ARGUMENT
    assert "twice" in _lib.last_error(ks[0]._h)
    assert lib.agbnp_hip_energy_group(hs, 2, pos, vp([bufs[0].ene.data_ptr(), 0]), None) == _lib.ERR_INVALID_ARGUMENT
    assert lib.agbnp_hip_energy_group(hs, 2, vp([bufs[0].pos.data_ptr(), 0]), ene, None) == _lib.ERR_INVALID_ARGUMENT
    assert lib.agbnp_hip_energy_group((C.c_void_p * 2)(ks[0]._h, None), 2, pos, ene, None) == _lib.ERR_INVALID_ARGUMENT
    overlap = vp([bufs[0].ene.data_ptr(), bufs[0].ene.data_ptr()])
    assert lib.agbnp_hip_energy_group(hs, 2, pos, overlap, None) == _lib.ERR_INVALID_ARGUMENT
    assert "overlap" in _lib.last_error(ks[0]._h)
    shared_pos = vp([bufs[0].pos.data_ptr(), bufs[0].pos.data_ptr()])  # (position buffers MAY be shared: accepted below)
    geoms = [s.jittered(20), s.jittered(20)]
    for b, g2 in zip(bufs, geoms):
        b.load(g2)
    assert lib.agbnp_hip_energy_group(hs, 2, shared_pos, ene, C.c_void_p(stream)) == _lib.OK
    # every member has ONE evaluation enqueued since its last finish: the refused calls counted nothing
    assert [k.wait_verdict(0, timeout=30.0) for k in ks] == [(1, 0), (1, 0)]
    assert [k.poll() for k in ks] == [(1, 0), (1, 0)]
    assert [k.finish(stream) for k in ks] == [0, 0]
    assert [list(k.withheld()) for k in ks] == [[], []]
    for b, g2 in zip(bufs, geoms):
        _energy_close(b.result()[0], oracle.execute(g2)[0])


def test_energy_group_host_repeats_a_jump_inside(gpu_required, systems, five):
    """Host buffers: one member jumps in the last round; the repeat happens inside and every member matches its oracle."""
    s, d = systems("trpcage"), systems("1dwc")
    members = [(s, 1), (d, 1), (s, 0)]
    ks = [_kernel(x.params(), v) for x, v in members]
    oracles = [Oracle(*x.params(), version=v) for x, v in members]
    for step in range(3):
        geoms = [x.jittered(step + 5 * m) for m, (x, _) in enumerate(members)]
        if step == 2:
            geoms[0] = geoms[0] + np.array([0.0, 0.1, 0.0])
        energies = P.energy_group_host(ks, geoms)
        for e, o, g in zip(energies, oracles, geoms):
            _energy_close(e, o.execute(g)[0])


def test_cpp_mirror_runs_an_energy_group(gpu_required, systems, five, tmp_path):
    """tests/cxx/TestHipEnergyGroup.cpp through cpp/AGBNPForce.h: energyGroup agrees with each context's energy(), and
    expectJump() in front of a far geometry gives a complete first evaluation."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(root, "openmm_agbnp_plugin_amd")
    exe = str(tmp_path / "TestHipEnergyGroup")
    subprocess.run(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", os.path.join(root, "tests", "cxx", "TestHipEnergyGroup.cpp"),
                    "-o", exe, os.path.join(libdir, "libagbnp_hip.so"), "-L/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{libdir}",
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    files = []
    for name in ("trpcage", "1dwc"):
        x = systems(name)
        path = tmp_path / f"{name}.txt"
        r, g, a, q, h = x.params()
        np.savetxt(path, np.column_stack([r, g, a, q, np.asarray(h, dtype=float), x.pos]), fmt="%.17g")
        files.append(str(path))
    out = subprocess.run([exe] + files, capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr


def _egroup_until_complete(ks, bufs, geoms, stream, attempts=8):
    """One energy-group evaluation of every member; withheld members (a capacity climb) are repeated through a group of those, as
    a caller of energy_device repeats them.  Returns how many group calls it took."""
    todo = list(range(len(ks)))
    for call in range(1, attempts + 1):
        for m in todo:
            bufs[m].load(geoms[m], SENTINEL)
        _egroup([ks[m] for m in todo], [bufs[m] for m in todo], stream)
        withheld = [m for m in todo if ks[m].finish(stream)]
        for m in todo:
            e, f = bufs[m].result()
            assert (f == SENTINEL).all()
            if m in withheld:
                assert e == 0.0, "a withheld member's energy word received something"
            else:
                assert e != 0.0
        if not withheld:
            return call
        todo = withheld
    raise AssertionError("the capacity negotiation did not converge")


@pytest.mark.parametrize("spacing,variant", [(0.24, 2), (0.22, 3)])
def test_members_that_climb_a_capacity_variant_form_their_own_launch_set(gpu_required, systems, five, monkeypatch, spacing, variant):
    """Two dense clusters in an energy group with two trpcage members: their geometry needs a larger capacity variant, so their
    first evaluation is withheld and their contexts climb (scalar 6); the repeat and every evaluation after it are right, the
    two clusters share the energy-only launches of their variant while the trpcage members keep sharing theirs."""
    torch = pytest.importorskip("torch")
    monkeypatch.setenv("AGBNP_HIP_SPLIT_FIT", "0")  # (every subtree whole: the variant's own kernels run, as in test_gpu_parity)
    tp, cl = systems("trpcage"), _cluster(150, spacing, 1)
    members = [tp, cl, tp, cl]
    ks = [_kernel(x.params()) for x in members]
    oracles = {id(x): Oracle(*x.params(), version=1) for x in (tp, cl)}
    stream = torch.cuda.current_stream().cuda_stream
    bufs = [Buffers(torch, x.n) for x in members]
    _egroup_until_complete(ks, bufs, [x.jittered(m) for m, x in enumerate(members)], stream)
    assert [int(k.scalar("variant")) for k in ks] == [0, variant, 0, variant]  # (every context starts on variant 0)
    for step in range(1, 4):
        geoms = [x.jittered(10 * step + m) for m, x in enumerate(members)]
        assert _egroup_until_complete(ks, bufs, geoms, stream) == 1
        for b, x, g in zip(bufs, members, geoms):
            _energy_close(b.result()[0], oracles[id(x)].execute(g)[0])
        assert _members(ks) == [2, 2, 2, 2]
        assert _kinds(ks) == [1, 1, 1, 1]
    assert [int(k.scalar("variant")) for k in ks] == [0, variant, 0, variant]


def test_far_strip_members_share_their_own_gb_launch(gpu_required, systems, five, monkeypatch):
    """AGBNP_HIP_GB_FAR=1 selects the GB instantiation with the far-strip test: two such members share its energy-only group
    launch and are right; a member created without it forms another launch set."""
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    oracle = Oracle(*s.params(), version=1)
    monkeypatch.setenv("AGBNP_HIP_GB_FAR", "1")
    far = [_kernel(s.params()) for _ in range(2)]
    monkeypatch.setenv("AGBNP_HIP_GB_FAR", "0")
    near = _kernel(s.params())
    ks = far + [near]
    stream = torch.cuda.current_stream().cuda_stream
    bufs = [Buffers(torch, s.n) for _ in ks]
    for step in range(4):
        geoms = [s.jittered(5 * step + m) for m in range(3)]
        assert _egroup_until_complete(ks, bufs, geoms, stream) == 1
        for b, g in zip(bufs, geoms):
            _energy_close(b.result()[0], oracle.execute(g)[0])
    assert _members(ks) == [2, 2, 1]
    assert _kinds(ks) == [1, 1, 1]
