"""GPU box: decomposition groups (include/agbnp_hip.h: agbnp_hip_decompose_group / _host).  Every member of a
group must get what its own agbnp_hip_decompose_device would give it: every one of its 4 N terms is the restatement's
(tests/decomposition_restatement.py, TIGHT) and that of a twin context evaluated alone (SAME = 1e-9, the twin tolerance of
DESIGN s.4n), its total is the oracle's, its verdict and its overflow log are its own, and it is left as an energy-only
evaluation leaves it.  The restatement of a geometry is computed once and shared (REFS)."""
import ctypes as C

import numpy as np
import pytest

import openmm_agbnp_plugin_amd as P
from openmm_agbnp_plugin_amd import _lib
from oracle import Oracle
from tests.decomposition_restatement import restate
from tests.edge_systems import edge_systems
from tests.gpu_helpers import SAME, TIGHT, Buffers
from tests.gpu_helpers import close as _close
from tests.gpu_helpers import energy_close as _energy_close
from tests.gpu_helpers import execute_group as _fgroup
from tests.gpu_helpers import five_groups as five  # noqa: F401

pytestmark = pytest.mark.gpu
SENTINEL = -1234.5678
JUMP = 16  # scalar 15: the evaluation was void because heavy atoms had left the neighbour masks' skin
REFS = {}
WORST = [0.0]  # the worst |term - restatement| this file has seen (printed by every comparison)


def reference(s, tag, pos, version=1, cutoff=None):
    """(energy, terms[4, N]) of the restatement at `pos`, once per (system, tag, version, cutoff)."""
    key = (s.name, tag, version, cutoff)
    if key not in REFS:
        e, terms, _ = restate(s.params(), pos, version=version, cutoff=cutoff)
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


def terms_close(terms, ref, tol=TIGHT, what="restatement"):
    assert terms.shape == ref.shape
    worst = np.abs(terms - ref).max(axis=1)
    if what == "restatement":
        WORST[0] = max(WORST[0], float(worst.max()))
    print(f"worst |term - {what}| per plane: {worst}  (file so far, against the restatement: {WORST[0]:.3e})")
    assert worst.max() < tol, f"terms differ from the {what} by {worst} (planes cavity, vdw, gb_self, gb_pair)"


class Planes:
    """Device positions, planes and total of one member."""

    def __init__(self, torch, n, fill=0.0, efill=0.0):
        dev = torch.device("cuda:0")
        self.torch, self.n = torch, n
        self.pos = torch.zeros((n, 3), dtype=torch.float64, device=dev)
        self.terms = torch.full((4, n), fill, dtype=torch.float64, device=dev)
        self.ene = torch.full((1,), efill, dtype=torch.float64, device=dev)

    def load(self, geom, fill=0.0, efill=0.0):
        self.pos.copy_(self.torch.tensor(np.asarray(geom), dtype=self.torch.float64))
        self.terms.fill_(fill)
        self.ene.fill_(efill)

    def result(self):
        return self.ene.item(), self.terms.cpu().numpy()


def _dgroup(kernels, bufs, stream, energies=True):
    P.decompose_group(kernels, [b.pos.data_ptr() for b in bufs], [b.terms.data_ptr() for b in bufs],
                      [b.ene.data_ptr() for b in bufs] if energies else None, stream)


def _egroup(kernels, bufs, stream):
    P.energy_group(kernels, [b.pos.data_ptr() for b in bufs], [b.ene.data_ptr() for b in bufs], stream)


def _kinds(ks):
    return [int(k.scalar("last_evaluation_kind")) for k in ks]


def _members(ks):
    return [int(k.scalar("group_members")) for k in ks]


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


def group_and_twins(torch, members, geoms, tags, expect_members=None, twin_tol=SAME):
    """members: (system, version, mode, cutoff) each.  One decomposition group over kernels of them at `geoms`, and every
    member's own decompose_device on a twin context: every term the restatement's and the twin's.  A first evaluation that is
    withheld for a capacity climb is repeated the way a caller repeats: the same call again."""
    stream = _stream(torch)
    ks = [_kernel(s, v, mode, cut) for s, v, mode, cut in members]
    twins = [_kernel(s, v, mode, cut) for s, v, mode, cut in members]
    bufs = [Planes(torch, s.n) for s, _, _, _ in members]
    tb = [Planes(torch, s.n) for s, _, _, _ in members]
    for attempt in range(4):
        for b, t, g in zip(bufs, tb, geoms):
            b.load(g)
            t.load(g)
        _dgroup(ks, bufs, stream)
        for tw, t in zip(twins, tb):
            tw.decompose_device(t.pos.data_ptr(), t.terms.data_ptr(), t.ene.data_ptr(), stream)
        withheld = [k.finish(stream) for k in ks]
        assert [k.finish(stream) for k in twins] == withheld  # (a member is withheld exactly when it is withheld alone)
        for w, b in zip(withheld, bufs):
            if w:
                assert not b.terms.any().item() and b.ene.item() == 0.0
        if not any(withheld):
            break
    assert not any(withheld), [(k.withheld(), int(k.scalar("overflow_kinds"))) for k in ks]
    assert _kinds(ks) == [3] * len(ks)
    if expect_members is not None:
        assert _members(ks) == expect_members
    for (s, v, _, cut), b, t, g, tag in zip(members, bufs, tb, geoms, tags):
        e_ref, ref = reference(s, tag, g, v, cut)
        e, terms = b.result()
        te, tt = t.result()
        terms_close(terms, ref)
        terms_close(terms, tt, twin_tol, "twin")
        _energy_close(e, e_ref)
        _energy_close(e, te, tol=SAME)
        _energy_close(float(terms.sum()), e_ref)
    return ks


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------
def test_four_trpcage_geometries_in_one_group(gpu_required, systems, five):
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    group_and_twins(torch, [(s, 1, "reference", None)] * 4, [s.jittered(m) for m in range(4)], [f"jitter{m}" for m in range(4)], [4] * 4)


def test_block_edges_and_member_boundaries_inside_one_grid(gpu_required, five):
    """One partial block; a second block of one atom; odd block counts with last blocks of one atom: the edges of decompose_tile,
    with members of 1, 3, 15 and 45 tiles side by side in the plane launch's grid."""
    torch = pytest.importorskip("torch")
    edge = edge_systems()
    members = [(edge[name], 1, "reference", None) for name in ("size_1_33", "size_65_65", "size_129_257", "size_257_513")]
    ks = group_and_twins(torch, members, [m[0].pos for m in members], ["file"] * 4)
    for k in ks:  # (members that climbed to the same capacity variant share a set; nobody ran outside the group's launches)
        same = sum(1 for j in ks if int(j.scalar("variant")) == int(k.scalar("variant")))
        assert int(k.scalar("group_members")) == same


def test_version_0_and_version_1_members_make_two_launch_sets(gpu_required, systems, five):
    torch = pytest.importorskip("torch")
    s, f = systems("trpcage"), systems("fixture264")
    members = [(s, 1, "reference", None), (s, 0, "reference", None), (f, 0, "reference", None), (s, 1, "reference", None)]
    geoms = [s.jittered(1), s.jittered(2), f.pos, s.jittered(3)]
    ks = group_and_twins(torch, members, geoms, ["jitter1", "jitter2", "file", "jitter3"], [2, 2, 2, 2])
    assert [int(k.scalar("energy_only_launches")) + 1 for k in ks] == [5, 3, 3, 5]  # launches of each member's launch set


def test_members_that_cannot_share_run_alone_and_everyone_is_right(gpu_required, systems, five):
    """A fast-mode member with a cutoff and a fast+single member (FP64 terms: the single-precision option lifted for the call)
    among Reference members: the two run what decompose_device runs for them, the others share; fast+single stays in its mode."""
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    members = [(s, 1, "reference", None), (s, 1, "fast", 1.0), (s, 1, "fast+single", 1.0), (s, 1, "reference", None)]
    ks = group_and_twins(torch, members, [s.jittered(m) for m in range(4)], [f"jitter{m}" for m in range(4)], [2, 0, 0, 2])
    single = ks[2]
    before = single.energy(s.pos)
    assert abs(before - reference(s, "file", s.pos, 1, 1.0)[0]) < 0.1 and abs(single.energy(s.pos) - before) < 1e-6
    assert P.HipCalcAGBNPForceKernel.MODES["fast+single"] == _lib.load().agbnp_hip_get_mode(single._h)


def test_a_once_captured_member(gpu_required, systems, five):
    """A member whose set the device names (captured into a graph and replayed once) runs alone inside the group, the sv_large
    cavity instantiation with the device's parity, and is right beside two members that share."""
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    stream = _stream(torch)
    ks = [_kernel(s) for _ in range(3)]
    cap = Buffers(torch, s.n)
    cap.load(s.jittered(9))
    ks[1].execute(s.pos, np.zeros((s.n, 3)))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ks[1].execute_device(*cap.ptrs(), torch.cuda.current_stream().cuda_stream)
    g.replay()
    torch.cuda.synchronize()
    assert ks[1].finish(stream) == 0
    bufs = [Planes(torch, s.n) for _ in ks]
    for rnd in range(2):  # (both parities of the device's count)
        geoms = [s.jittered(10 * rnd + m) for m in range(3)]
        for b, gm in zip(bufs, geoms):
            b.load(gm)
        _dgroup(ks, bufs, stream)
        assert [k.finish(stream) for k in ks] == [0, 0, 0]
        assert _members(ks) == [2, 0, 2] and _kinds(ks) == [3, 3, 3]
        for b, gm, m in zip(bufs, geoms, range(3)):
            e_ref, ref = reference(s, f"jitter{10 * rnd + m}", gm)
            e, terms = b.result()
            terms_close(terms, ref)
            _energy_close(e, e_ref)


def test_sixteen_members(gpu_required, five):
    torch = pytest.importorskip("torch")
    s = edge_systems()["size_65_65"]
    rng = np.random.default_rng(7)
    geoms = [s.pos] + [s.pos + rng.normal(0.0, 0.002, s.pos.shape) for _ in range(15)]
    ks = group_and_twins(torch, [(s, 1, "reference", None)] * 16, geoms, ["file"] + [f"rng7_{m}" for m in range(1, 16)])
    assert _members(ks) == [16] * 16


def test_group_launches_switched_off(gpu_required, systems, five, monkeypatch):
    torch = pytest.importorskip("torch")
    monkeypatch.setenv("AGBNP_HIP_GROUP_LAUNCHES", "0")
    s = systems("trpcage")
    group_and_twins(torch, [(s, 1, "reference", None)] * 3, [s.jittered(m) for m in range(3)], [f"jitter{m}" for m in range(3)], [0, 0, 0])


# ---- 2. the device call adds; the host call overwrites -----------------------------------------------------------------------
def test_the_device_call_adds_and_takes_no_energy_words(gpu_required, systems, five):
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    stream = _stream(torch)
    ks = [_kernel(s) for _ in range(2)]
    bufs = [Planes(torch, s.n) for _ in ks]
    geoms = [s.jittered(1), s.jittered(2)]
    for b, g in zip(bufs, geoms):
        b.load(g, 1.0, 2.0)
    pos0 = [b.pos.clone() for b in bufs]
    _dgroup(ks, bufs, stream)
    _dgroup(ks, bufs, stream)
    _dgroup(ks, bufs, stream, energies=False)  # d_energies = NULL is accepted
    assert [k.finish(stream) for k in ks] == [0, 0]
    assert _members(ks) == [2, 2]
    for b, g, tag, p0 in zip(bufs, geoms, ("jitter1", "jitter2"), pos0):
        e_ref, ref = reference(s, tag, g)
        e, terms = b.result()
        terms_close(terms, 1.0 + 3.0 * ref, 3 * TIGHT)
        _energy_close(e, 2.0 + 2.0 * e_ref, 2 * TIGHT)
        assert torch.equal(b.pos, p0)


def test_the_host_form_overwrites_and_repeats_a_jumped_member(gpu_required, systems, five):
    s, f = systems("trpcage"), systems("fixture264")
    ks = [_kernel(s), _kernel(f, 0), _kernel(s)]
    energies, terms = P.decompose_group_host(ks, [s.jittered(1), f.pos, s.jittered(2)])
    for e, t, (x, tag, g, v) in zip(energies, terms, [(s, "jitter1", s.jittered(1), 1), (f, "file", f.pos, 0), (s, "jitter2", s.jittered(2), 1)]):
        e_ref, ref = reference(x, tag, g, v)
        terms_close(t, ref)
        _energy_close(e, e_ref)
    moved = s.jittered(3) + np.array([0.1, 0.0, 0.0])  # (the third member jumps: withheld on the device, repeated inside)
    energies, terms = P.decompose_group_host(ks, [s.jittered(4), f.pos, moved])
    for e, t, (x, tag, g, v) in zip(energies, terms, [(s, "jitter4", s.jittered(4), 1), (f, "file", f.pos, 0), (s, "moved3", moved, 1)]):
        e_ref, ref = reference(x, tag, g, v)
        terms_close(t, ref)
        _energy_close(e, e_ref)


# ---- 3. withheld -------------------------------------------------------------------------------------------------------------
def test_a_jump_is_withheld_for_that_member_only(gpu_required, systems, five):
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    stream = _stream(torch)
    ks = [_kernel(s) for _ in range(3)]
    bufs = [Planes(torch, s.n) for _ in ks]
    for b, m in zip(bufs, range(3)):
        b.load(s.jittered(m))
    _dgroup(ks, bufs, stream)
    assert [k.finish(stream) for k in ks] == [0, 0, 0]
    geoms = [s.jittered(10 + m) for m in range(3)]
    geoms[1] = geoms[1] + np.array([0.1, 0.0, 0.0])
    for b, g in zip(bufs, geoms):
        b.load(g, SENTINEL, SENTINEL)
    _dgroup(ks, bufs, stream)
    assert [k.finish(stream) for k in ks] == [0, 1, 0]
    assert list(ks[1].withheld()) == [0] and int(ks[1].scalar("overflow_kinds")) & JUMP
    e, terms = bufs[1].result()
    assert e == SENTINEL and (terms == SENTINEL).all()  # bit-unchanged
    for m in (0, 2):
        e_ref, ref = reference(s, f"jitter{10 + m}", geoms[m])
        e, terms = bufs[m].result()
        terms_close(terms - SENTINEL, ref)
        _energy_close(e - SENTINEL, e_ref)
    e_ref, ref = reference(s, "jitter11_moved", geoms[1])
    bufs[1].load(geoms[1])
    _dgroup(ks, bufs[:1] + bufs[1:2] + bufs[2:], stream)  # the repeat, through the whole group again
    assert [k.finish(stream) for k in ks] == [0, 0, 0]
    e, terms = bufs[1].result()
    terms_close(terms, ref)
    _energy_close(e, e_ref)
    back = s.jittered(12)  # 0.1 nm back: a jump again, not withheld with the hint
    ks[1].expect_jump()
    bufs[1].load(back)
    _dgroup(ks, bufs, stream)
    assert [k.finish(stream) for k in ks] == [0, 0, 0]
    terms_close(bufs[1].result()[1], reference(s, "jitter12", back)[1])


# ---- 4. interleaving and launches --------------------------------------------------------------------------------------------
def test_the_three_group_kinds_interleaved_rewrite_no_block(gpu_required, systems, five):
    """execute_group, energy_group and decompose_group of the same three members with fixed position buffers, round after round:
    every result is right, and after the second round -- both parities of every member met -- no argument block is rewritten."""
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    oracle = Oracle(*s.params(), version=1)
    stream = _stream(torch)
    ks = [_kernel(s) for _ in range(3)]
    bufs = [Buffers(torch, s.n) for _ in ks]
    planes = [torch.zeros((4, s.n), dtype=torch.float64, device=torch.device("cuda:0")) for _ in ks]
    settled = None
    step = 0
    for rnd in range(4):
        for what in "FED":
            geoms = [s.jittered(40 * m + step) for m in range(3)]
            for b, g, p in zip(bufs, geoms, planes):
                b.load(g, SENTINEL if what != "F" else 0.0)
                p.zero_()
            if what == "F":
                _fgroup(ks, bufs, stream)
            elif what == "E":
                _egroup(ks, bufs, stream)
            else:
                P.decompose_group(ks, [b.pos.data_ptr() for b in bufs], [p.data_ptr() for p in planes], [b.ene.data_ptr() for b in bufs], stream)
            assert [k.finish(stream) for k in ks] == [0, 0, 0]
            assert _kinds(ks) == [dict(F=0, E=1, D=3)[what]] * 3 and _members(ks) == [3, 3, 3]
            for m, (b, g, p) in enumerate(zip(bufs, geoms, planes)):
                e, f = b.result()
                eo, fo = oracle.execute(g)
                if what == "F":
                    _close(e, f, eo, fo)
                else:
                    assert (f == SENTINEL).all(), "a force buffer was written"
                    _energy_close(e, eo)
                if what == "D":
                    terms_close(p.cpu().numpy(), reference(s, f"jitter{40 * m + step}", g)[1])
                else:
                    assert not p.any().item()
            step += 1
        writes = [int(k.scalar("group_block_writes")) for k in ks]
        print("round", rnd, "group_block_writes", writes)
        if rnd == 1:
            settled = writes
        if rnd > 1:
            assert writes == settled, "a steady run of mixed group calls rewrote an argument block"
    assert settled == [2, 2, 2]  # (one write per parity, whichever kind of call met it first)


@pytest.mark.parametrize("version", [1, 0])
@pytest.mark.parametrize("R", [2, 8])
def test_a_launch_set_costs_five_launches_whatever_its_size(gpu_required, systems, five, version, R):
    """All R members ran in ONE launch set (scalar 19 = R) as decompositions (scalar 20 = 3): the energy-only group's launches
    (scalar 18: four, version 0 two) and the one plane launch -- 5 (3) for the set, where R decompose_device calls make 5 R."""
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    ks = group_and_twins(torch, [(s, version, "reference", None)] * R, [s.jittered(m) for m in range(R)],
                         [f"jitter{m}" for m in range(R)], [R] * R)
    assert [int(k.scalar("energy_only_launches")) + 1 for k in ks] == [5 if version == 1 else 3] * R


# ---- 5. refusals: argument checks that return before any launch --------------------------------------------------------------
def test_the_refusals(gpu_required, systems, five):
    torch = pytest.importorskip("torch")
    lib = _lib.load()
    s = systems("trpcage")
    stream = _stream(torch)
    ks = [_kernel(s) for _ in range(2)]
    bufs = [Planes(torch, s.n) for _ in ks]
    for b, m in zip(bufs, range(2)):
        b.load(s.jittered(m), SENTINEL, SENTINEL)
    pos, terms, ene = ([b.pos.data_ptr() for b in bufs], [b.terms.data_ptr() for b in bufs], [b.ene.data_ptr() for b in bufs])
    # 17 members: the wrapper refuses, and so does the library itself
    with pytest.raises(P.OpenMMException, match="1 to 16"):
        P.decompose_group([ks[0]] * 17, pos[:1] * 17, terms[:1] * 17, None, stream)
    arr = C.c_void_p * 17
    handles, p17 = arr(*[ks[0]._h] * 17), arr(*[pos[0]] * 17)
    assert lib.agbnp_hip_decompose_group(handles, 17, p17, p17, None, None) == _lib.ERR_INVALID_ARGUMENT
    assert "1 to 16" in _lib.last_error(ks[0]._h)
    with pytest.raises(P.OpenMMException, match="twice"):
        P.decompose_group([ks[0], ks[0]], pos, terms, ene, stream)
    # plane spans [4 n] that overlap: by one word, and an energy word inside another member's planes
    with pytest.raises(P.OpenMMException, match="plane buffers of two members overlap"):
        P.decompose_group(ks, pos, [terms[0], terms[0] + 8 * (4 * s.n - 1)], ene, stream)
    with pytest.raises(P.OpenMMException, match="plane buffers of two members overlap"):
        P.decompose_group(ks, pos, terms, [terms[1] + 8, ene[1]], stream)
    with pytest.raises(P.OpenMMException, match="energy words of two members overlap"):
        P.decompose_group(ks, pos, terms, [ene[0], ene[0]], stream)
    with pytest.raises(P.OpenMMException, match="null pointer"):
        P.decompose_group(ks, pos, [terms[0], 0], ene, stream)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        bufs[0].ene.fill_(1.0)
        with pytest.raises(P.OpenMMException, match="captur"):
            _dgroup(ks, bufs, torch.cuda.current_stream().cuda_stream)
    g.replay()
    torch.cuda.synchronize()
    # nothing was launched, no member changed: no evaluation in any log, the buffers as they were, and the group works
    assert [k.finish(stream) for k in ks] == [0, 0]
    assert bufs[0].ene.item() == 1.0 and bufs[1].ene.item() == SENTINEL
    assert all((b.terms == SENTINEL).all().item() for b in bufs)
    for b, m in zip(bufs, range(2)):
        b.load(s.jittered(m))
    _dgroup(ks, bufs, stream)
    assert [k.finish(stream) for k in ks] == [0, 0]
    for b, m in zip(bufs, range(2)):
        terms_close(b.result()[1], reference(s, f"jitter{m}", s.jittered(m))[1])
