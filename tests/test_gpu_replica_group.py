"""GPU box: replica groups (include/agbnp_hip.h: agbnp_hip_execute_group / _host) -- several contexts evaluated
in one call, the members that can share their launches launched once per stage.  Every member must get what its own
agbnp_hip_execute_device would give it: the oracle's numbers, the numbers of a twin context evaluated alone, its own overflow log."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import openmm_agbnp_plugin_amd as P
from openmm_agbnp_plugin_amd import _lib
from oracle import Oracle
from tests.gpu_helpers import SAME, TIGHT, Buffers
from tests.gpu_helpers import close as _close
from tests.gpu_helpers import cluster as _cluster
from tests.gpu_helpers import execute_group as _group
from tests.gpu_helpers import five_groups as five  # noqa: F401
from tests.gpu_helpers import kernel_of as _kernel

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("version,name", [(1, "trpcage"), (1, "1dwc"), (1, "fixture264"), (0, "trpcage")])
@pytest.mark.parametrize("R", [1, 2, 4])
def test_group_matches_the_oracle_and_twins_alone(gpu_required, systems, five, version, name, R):
    """R contexts of one system, each on a jittered trajectory of its own: every member's energy and forces are the oracle's and
    those of a twin context evaluated alone through execute_device; the members share one launch set."""
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
            b.load(g)
            t.load(g)
        _group(ks, bufs, stream)
        for tw, t in zip(twins, tb):
            tw.execute_device(*t.ptrs(), stream)
        for m in range(R):
            withheld = ks[m].finish(stream)
            assert twins[m].finish(stream) == withheld
            if withheld:  # (a capacity climb: repeated through the group, as a caller of execute_device repeats)
                bufs[m].load(geoms[m])
                _group([ks[m]], [bufs[m]], stream)
                assert ks[m].finish(stream) == 0
                tb[m].load(geoms[m])
                twins[m].execute_device(*tb[m].ptrs(), stream)
                assert twins[m].finish(stream) == 0
            e, f = bufs[m].result()
            _close(e, f, *oracle.execute(geoms[m]))
            _close(e, f, *tb[m].result(), tol=SAME)
        shared = [int(k.scalar("variant")) <= 3 for k in ks]
        if all(shared):
            assert [int(k.scalar("group_members")) for k in ks] == [R] * R


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
        _group(ks, bufs, stream)
        assert [k.finish(stream) for k in ks] == [0] * len(ks)
        for b, o, g in zip(bufs, oracles, geoms):
            _close(*b.result(), *o.execute(g))
    assert int(ks[3].scalar("group_members")) == 1
    v1 = [k for (_, _, v), k in zip(members, ks) if v == 1]
    for k in v1:
        same = sum(1 for j in v1 if int(j.scalar("variant")) == int(k.scalar("variant")))
        assert int(k.scalar("group_members")) == same


def test_members_that_cannot_share_run_alone(gpu_required, systems, five):
    """A deterministic-mode member and a member with diagnostics run their own launches (scalar 19 = 0) and are right; the two
    others still share."""
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    oracle = Oracle(*s.params(), version=1)
    ks = [_kernel(s.params()), _kernel(s.params(), mode="deterministic"), _kernel(s.params()), _kernel(s.params())]
    _lib.load().agbnp_hip_set_diagnostics(ks[2]._h, 1)
    stream = torch.cuda.current_stream().cuda_stream
    bufs = [Buffers(torch, s.n) for _ in ks]
    for step in range(3):
        geoms = [s.jittered(step + 11 * m) for m in range(len(ks))]
        for b, g in zip(bufs, geoms):
            b.load(g)
        _group(ks, bufs, stream)
        assert [k.finish(stream) for k in ks] == [0] * len(ks)
        for b, g in zip(bufs, geoms):
            _close(*b.result(), *oracle.execute(g))
    assert [int(k.scalar("group_members")) for k in ks] == [2, 0, 0, 2]


def test_a_jump_is_withheld_for_that_member_only(gpu_required, systems, five):
    """One member jumps 0.1 nm: only its finish() reports a withheld evaluation and its buffers received nothing; the others are
    complete and right.  Its repeat, through a group and through a single call, is right."""
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    oracle = Oracle(*s.params(), version=1)
    ks = [_kernel(s.params()) for _ in range(3)]
    stream = torch.cuda.current_stream().cuda_stream
    bufs = [Buffers(torch, s.n) for _ in ks]
    geoms = [s.jittered(m) for m in range(3)]
    for b, g in zip(bufs, geoms):
        b.load(g)
    _group(ks, bufs, stream)
    assert [k.finish(stream) for k in ks] == [0, 0, 0]
    geoms = [s.jittered(10 + m) for m in range(3)]
    geoms[1] = geoms[1] + np.array([0.1, 0.0, 0.0])
    for b, g in zip(bufs, geoms):
        b.load(g)
    _group(ks, bufs, stream)
    assert [k.finish(stream) for k in ks] == [0, 1, 0]
    assert list(ks[1].withheld()) == [0]
    e1, f1 = bufs[1].result()
    assert e1 == 0.0 and not f1.any()
    for m in (0, 2):
        _close(*bufs[m].result(), *oracle.execute(geoms[m]))
    bufs[1].load(geoms[1])
    _group([ks[1]], [bufs[1]], stream)  # the repeat through a group ...
    assert ks[1].finish(stream) == 0
    _close(*bufs[1].result(), *oracle.execute(geoms[1]))
    jump = geoms[1] - np.array([0.1, 0.0, 0.0])
    bufs[1].load(jump)
    _group(ks[1:2], bufs[1:2], stream)
    assert ks[1].finish(stream) == 1
    bufs[1].load(jump)
    ks[1].execute_device(*bufs[1].ptrs(), stream)  # ... and through a single call
    assert ks[1].finish(stream) == 0
    _close(*bufs[1].result(), *oracle.execute(jump))


def test_group_and_single_calls_interleave(gpu_required, systems, five):
    """Group calls mixed with execute_device, execute_host and energy_device on the same contexts in an irregular order, with the
    NULL stream: every result is the oracle's."""
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    oracle = Oracle(*s.params(), version=1)
    ks = [_kernel(s.params()) for _ in range(3)]
    bufs = [Buffers(torch, s.n) for _ in ks]
    plan = ["group", "device", "group", "host", "energy", "group", "group", "host", "device", "group"]
    for step, what in enumerate(plan):
        geoms = [s.jittered(3 * step + m) for m in range(3)]
        for b, g in zip(bufs, geoms):
            b.load(g)
        torch.cuda.synchronize()
        if what == "group":
            _group(ks, bufs, None)
        for m, k in enumerate(ks):
            if what == "device":
                k.execute_device(*bufs[m].ptrs(), None)
            elif what == "energy":
                k.energy_device(bufs[m].pos.data_ptr(), bufs[m].ene.data_ptr(), None)
            elif what == "host":
                f = np.zeros((s.n, 3))
                _close(k.execute(geoms[m], f), f, *oracle.execute(geoms[m]))
                continue
            assert k.finish(None) == 0
            e, f = bufs[m].result()
            eo, fo = oracle.execute(geoms[m])
            if what == "energy":
                assert abs(e - eo) < TIGHT * max(1.0, abs(eo) * 1e-3)
            else:
                _close(e, f, eo, fo)


def test_refusals_change_nothing(gpu_required, systems, five):
    """Inside a stream capture the call is refused and the capture still completes; count 0 or 17, a NULL pointer and the same
    context twice are refused; the members' next evaluation is right."""
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    oracle = Oracle(*s.params(), version=1)
    ks = [_kernel(s.params()) for _ in range(2)]
    stream = torch.cuda.current_stream().cuda_stream
    bufs = [Buffers(torch, s.n) for _ in ks]
    for b, m in zip(bufs, range(2)):
        b.load(s.jittered(m))
    _group(ks, bufs, stream)
    assert [k.finish(stream) for k in ks] == [0, 0]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        bufs[0].ene.add_(1.0)
        with pytest.raises(P.OpenMMException):
            _group(ks, bufs, torch.cuda.current_stream().cuda_stream)
    g.replay()
    torch.cuda.synchronize()
    lib = _lib.load()
    hs = (C.c_void_p * 17)(*([ks[0]._h, ks[1]._h] * 9)[:17])
    vp = lambda ptrs: (C.c_void_p * len(ptrs))(*ptrs)  # noqa: E731
    pos, frc, ene = vp([b.pos.data_ptr() for b in bufs] * 9), vp([b.frc.data_ptr() for b in bufs] * 9), vp([b.ene.data_ptr() for b in bufs] * 9)
    assert lib.agbnp_hip_execute_group(hs, 0, pos, frc, ene, None) == _lib.ERR_INVALID_ARGUMENT
    assert lib.agbnp_hip_execute_group(hs, 17, pos, frc, ene, None) == _lib.ERR_INVALID_ARGUMENT
    twice = (C.c_void_p * 2)(ks[0]._h, ks[0]._h)
    assert lib.agbnp_hip_execute_group(twice, 2, pos, frc, ene, None) == _lib.ERR_INVALID_ARGUMENT
    assert "twice" in _lib.last_error(ks[0]._h)
    assert lib.agbnp_hip_execute_group(hs, 2, pos, vp([bufs[0].frc.data_ptr(), 0]), ene, None) == _lib.ERR_INVALID_ARGUMENT
    overlap = vp([bufs[0].frc.data_ptr(), bufs[0].frc.data_ptr() + 8])
    assert lib.agbnp_hip_execute_group(hs, 2, pos, overlap, ene, None) == _lib.ERR_INVALID_ARGUMENT
    geoms = [s.jittered(20 + m) for m in range(2)]
    for b, g2 in zip(bufs, geoms):
        b.load(g2)
    _group(ks, bufs, stream)
    assert [k.finish(stream) for k in ks] == [0, 0]
    for b, g2 in zip(bufs, geoms):
        _close(*b.result(), *oracle.execute(g2))


def test_execute_group_host_repeats_a_jump_inside(gpu_required, systems, five):
    """Host buffers: one member jumps; the repeat happens inside and every member matches its oracle; forces accumulate."""
    s, d = systems("trpcage"), systems("1dwc")
    members = [(s, 1), (d, 1), (s, 0)]
    ks = [_kernel(x.params(), v) for x, v in members]
    oracles = [Oracle(*x.params(), version=v) for x, v in members]
    for step in range(3):
        geoms = [x.jittered(step + 5 * m) for m, (x, _) in enumerate(members)]
        if step == 2:
            geoms[0] = geoms[0] + np.array([0.0, 0.1, 0.0])
        forces = [np.full((x.n, 3), 0.25) for x, _ in members]
        energies = P.execute_group_host(ks, geoms, forces)
        for e, f, o, g in zip(energies, forces, oracles, geoms):
            _close(e, f - 0.25, *o.execute(g))


def test_cpp_mirror_runs_a_group(gpu_required, systems, five, tmp_path):
    """tests/cxx/TestHipReplicaGroup.cpp through cpp/AGBNPForce.h: executeGroup agrees with each context's execute()."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(root, "openmm_agbnp_plugin_amd")
    exe = str(tmp_path / "TestHipReplicaGroup")
    subprocess.run(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", os.path.join(root, "tests", "cxx", "TestHipReplicaGroup.cpp"),
                    "-o", exe, os.path.join(libdir, "libagbnp_hip.so"), f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    files = []
    for name in ("trpcage", "1dwc"):
        x = systems(name)
        path = tmp_path / f"{name}.txt"
        r, g, a, q, h = x.params()
        np.savetxt(path, np.column_stack([r, g, a, q, np.asarray(h, dtype=float), x.pos]), fmt="%.17g")
        files.append(str(path))
    out = subprocess.run([exe] + files, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr


def _group_until_complete(ks, bufs, geoms, stream, attempts=8):
    """One group evaluation of every member; withheld members (a capacity climb) are repeated through a group of those, as a
    caller of execute_device repeats them.  Returns how many group calls it took."""
    todo = list(range(len(ks)))
    for call in range(1, attempts + 1):
        for m in todo:
            bufs[m].load(geoms[m])
        _group([ks[m] for m in todo], [bufs[m] for m in todo], stream)
        withheld = [m for m in todo if ks[m].finish(stream)]
        for m in todo:
            if m not in withheld:
                assert bufs[m].result()[0] != 0.0
        if not withheld:
            return call
        for m in withheld:
            e, f = bufs[m].result()
            assert e == 0.0 and not f.any(), "a withheld member's buffers received something"
        todo = withheld
    raise AssertionError("the capacity negotiation did not converge")


@pytest.mark.parametrize("spacing,variant", [(0.24, 2), (0.22, 3)])
def test_members_that_climb_a_capacity_variant_form_their_own_launch_set(gpu_required, systems, five, monkeypatch, spacing, variant):
    """Two dense clusters in a group with two trpcage members: their geometry needs a larger capacity variant, so their first
    evaluation is withheld and their contexts climb (scalar 6); the repeat and every evaluation after it are right, the two
    clusters share the launches of their variant (scalar 19 = 2: the group kernels of that variant, argument blocks rewritten
    for the new capacity) while the trpcage members keep sharing theirs."""
    torch = pytest.importorskip("torch")
    monkeypatch.setenv("AGBNP_HIP_SPLIT_FIT", "0")  # (every subtree whole: the variant's own kernels run, as in test_gpu_parity)
    tp, cl = systems("trpcage"), _cluster(150, spacing, 1)
    members = [tp, cl, tp, cl]
    ks = [_kernel(x.params()) for x in members]
    oracles = {id(x): Oracle(*x.params(), version=1) for x in (tp, cl)}
    stream = torch.cuda.current_stream().cuda_stream
    bufs = [Buffers(torch, x.n) for x in members]
    _group_until_complete(ks, bufs, [x.jittered(m) for m, x in enumerate(members)], stream)
    assert [int(k.scalar("variant")) for k in ks] == [0, variant, 0, variant]  # (every context starts on variant 0)
    for step in range(1, 4):
        geoms = [x.jittered(10 * step + m) for m, x in enumerate(members)]
        assert _group_until_complete(ks, bufs, geoms, stream) == 1
        for b, x, g in zip(bufs, members, geoms):
            _close(*b.result(), *oracles[id(x)].execute(g))
        assert [int(k.scalar("group_members")) for k in ks] == [2, 2, 2, 2]
    assert [int(k.scalar("variant")) for k in ks] == [0, variant, 0, variant]


def test_far_strip_members_share_their_own_gb_launch(gpu_required, systems, five, monkeypatch):
    """AGBNP_HIP_GB_FAR=1 selects the GB instantiation with the far-strip test: two such members share its group launch and are
    right; a member created without it forms another launch set."""
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
        assert _group_until_complete(ks, bufs, geoms, stream) == 1
        for b, g in zip(bufs, geoms):
            _close(*b.result(), *oracle.execute(g))
    assert [int(k.scalar("group_members")) for k in ks] == [2, 2, 1]


def test_changing_position_buffers_rewrites_the_blocks(gpu_required, systems, five):
    """A caller that hands a member another position buffer in every call (the argument block is rewritten each time) and other
    output buffers: every result is still the oracle's and the twin's alone."""
    torch = pytest.importorskip("torch")
    s = systems("1dwc")
    oracle = Oracle(*s.params(), version=1)
    ks = [_kernel(s.params()) for _ in range(2)]
    stream = torch.cuda.current_stream().cuda_stream
    pools = [[Buffers(torch, s.n) for _ in range(3)] for _ in ks]
    for step in range(7):
        bufs = [pools[m][(step * (m + 1)) % 3] for m in range(2)]
        geoms = [s.jittered(50 + 2 * step + m) for m in range(2)]
        assert _group_until_complete(ks, bufs, geoms, stream) == 1
        for b, g in zip(bufs, geoms):
            _close(*b.result(), *oracle.execute(g))
        assert [int(k.scalar("group_members")) for k in ks] == [2, 2]
