"""GPU box: pair-matrix groups (include/agbnp_hip.h: agbnp_hip_pair_matrix_group / _host).  Every member of a group
must get what its own agbnp_hip_pair_matrix_device would give it, over its own partition: every one of its S_m S_m cells is the
restatement's (tests/pair_matrix_restatement.py, TIGHT = 1e-7; `count` adds into one buffer: count x TIGHT) and that of a twin
context evaluated alone (SAME = 1e-9), its total is the oracle's (energy_close), its verdict and its overflow log are its own, and
it is left as an energy-only evaluation leaves it.  The restatement of a geometry is computed once, as the matrix of every atom
its own set, and shared with tests/test_gpu_pair_matrix.py (its `reference`)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import openmm_agbnp_plugin_amd as P
from openmm_agbnp_plugin_amd import _lib
from oracle import Oracle
from tests.edge_systems import edge_systems
from tests.gpu_helpers import SAME, TIGHT, Buffers
from tests.gpu_helpers import close as _close
from tests.gpu_helpers import energy_close as _energy_close
from tests.gpu_helpers import execute_group as _fgroup
from tests.gpu_helpers import five_groups as five  # noqa: F401
from tests.test_gpu_pair_matrix import PARTITIONS, _kernel, reference, residues

pytestmark = pytest.mark.gpu
SENTINEL = -1234.5678
JUMP = 16  # scalar 15: the evaluation was void because heavy atoms had left the neighbour masks' skin
WORST = [0.0]  # the worst |cell - restatement| this file has seen (printed by every comparison)


def cells_close(matrix, ref, tol=TIGHT, what="restatement", count=1):
    assert matrix.shape == ref.shape
    worst = float(np.abs(matrix - ref).max())
    if what == "restatement":
        WORST[0] = max(WORST[0], worst / count)
    print(f"worst |cell - {what}|: {worst:.3e} over {ref.shape[0]} x {ref.shape[1]} cells  (file so far, against the restatement, "
          f"per evaluation: {WORST[0]:.3e})")
    assert worst < tol, f"cells differ from the {what} by {worst:.3e}"


class Mats:
    """Device positions, matrix and total of one member."""

    def __init__(self, torch, n, S, fill=0.0, efill=0.0):
        dev = torch.device("cuda:0")
        self.torch, self.n = torch, n
        self.pos = torch.zeros((n, 3), dtype=torch.float64, device=dev)
        self.matrix = torch.full((S, S), fill, dtype=torch.float64, device=dev)
        self.ene = torch.full((1,), efill, dtype=torch.float64, device=dev)

    def load(self, geom, fill=0.0, efill=0.0):
        self.pos.copy_(self.torch.tensor(np.asarray(geom), dtype=self.torch.float64))
        self.matrix.fill_(fill)
        self.ene.fill_(efill)

    def result(self):
        return self.ene.item(), self.matrix.cpu().numpy()


def _mgroup(kernels, bufs, stream, energies=True):
    P.pair_matrix_group(kernels, [b.pos.data_ptr() for b in bufs], [b.matrix.data_ptr() for b in bufs],
                        [b.ene.data_ptr() for b in bufs] if energies else None, stream)


def _kinds(ks):
    return [int(k.scalar("last_evaluation_kind")) for k in ks]


def _members(ks):
    return [int(k.scalar("group_members")) for k in ks]


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


def _jumped(s, geom, by=0.06):
    """`geom` with one heavy atom moved by more than the masks' skin (0.04 nm)."""
    heavy = np.flatnonzero(s.ishydrogen == 0)
    moved = np.array(geom, copy=True)
    moved[heavy[len(heavy) // 2], 0] += by
    return moved


def group_and_twins(torch, members, geoms, tags, expect_members=None):
    """members: (system, version, mode, cutoff, sets, S) each.  One pair-matrix group over kernels of them at `geoms`, and every
    member's own pair_matrix_device on a twin context: every cell the restatement's and the twin's.  A first evaluation that is
    withheld for a capacity climb is repeated the way a caller repeats: the same call again."""
    stream = _stream(torch)
    ks = [_kernel(s, v, mode, cut, sets, S) for s, v, mode, cut, sets, S in members]
    twins = [_kernel(s, v, mode, cut, sets, S) for s, v, mode, cut, sets, S in members]
    bufs = [Mats(torch, m[0].n, m[5]) for m in members]
    tb = [Mats(torch, m[0].n, m[5]) for m in members]
    for attempt in range(4):
        for b, t, g in zip(bufs, tb, geoms):
            b.load(g)
            t.load(g)
        _mgroup(ks, bufs, stream)
        for tw, t in zip(twins, tb):
            tw.pair_matrix_device(t.pos.data_ptr(), t.matrix.data_ptr(), t.ene.data_ptr(), stream)
        withheld = [k.finish(stream) for k in ks]
        assert [k.finish(stream) for k in twins] == withheld  # (a member is withheld exactly when it is withheld alone)
        for w, b in zip(withheld, bufs):
            if w:
                assert not b.matrix.any().item() and b.ene.item() == 0.0
        if not any(withheld):
            break
    assert not any(withheld), [(k.withheld(), int(k.scalar("overflow_kinds"))) for k in ks]
    assert _kinds(ks) == [4] * len(ks)
    if expect_members is not None:
        assert _members(ks) == expect_members
    for (s, v, _, cut, sets, S), b, t, g, tag in zip(members, bufs, tb, geoms, tags):
        e_ref, ref = reference(s, tag, g, sets, S, version=v, cutoff=cut)
        e, m = b.result()
        te, tm = t.result()
        cells_close(m, ref)
        cells_close(m, tm, SAME, "twin")
        _energy_close(e, e_ref)
        _energy_close(e, te, tol=SAME)
        _energy_close(float(m.sum()), e_ref)
    return ks, bufs


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------
def test_three_partitions_of_trpcage_in_one_call(gpu_required, systems, five):
    """Residues (20 sets, about five to a block), every atom its own set (272 sets, the full 64 x 64 accumulator: the launch's
    dynamic LDS is this member's) and i % 3, at three geometries: one launch set, every member its own partition."""
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    sets, S = residues("trpcage")
    members = [(s, 1, "reference", None, sets, S), (s, 1, "reference", None, np.arange(s.n), s.n), (s, 1, "reference", None, np.arange(s.n) % 3, 3)]
    ks, _ = group_and_twins(torch, members, [s.jittered(m) for m in (1, 2, 3)], ["jitter1", "jitter2", "jitter3"], [3, 3, 3])
    assert [k.num_atom_sets() for k in ks] == [S, s.n, 3]
    assert [int(k.scalar("energy_only_launches")) + 1 for k in ks] == [5, 5, 5]  # launches of the one launch set


def test_members_of_different_sizes_side_by_side(gpu_required, five):
    """Members of 1, 3 and 15 tiles, each with sets across every block edge and with every other set empty, in one grid: a
    workgroup that picked the wrong member, or the wrong number inside its member's grid, adds to the wrong cells -- the odd rows
    and columns of the empty-set members must be exactly 0.0."""
    torch = pytest.importorskip("torch")
    edge = edge_systems()
    members = []
    for name in ("size_1_33", "size_65_65", "size_129_257"):
        for partition in ("straddling", "empty_sets"):
            sets, S = PARTITIONS[partition](edge[name].n)
            members.append((edge[name], 1, "reference", None, sets, S))
    ks, bufs = group_and_twins(torch, members, [m[0].pos for m in members], ["file"] * len(members))
    for k in ks:  # (members that climbed to the same capacity variant share a set; nobody ran outside the group's launches)
        same = sum(1 for j in ks if int(j.scalar("variant")) == int(k.scalar("variant")))
        assert int(k.scalar("group_members")) == same
    for b in bufs[1::2]:
        m = b.result()[1]
        assert (m[1::2] == 0.0).all() and (m[:, 1::2] == 0.0).all() and m[0::2, 0::2].any()


def test_a_version_0_member_forms_its_own_launch_set(gpu_required, systems, five):
    torch = pytest.importorskip("torch")
    s, f = systems("trpcage"), systems("fixture264")
    sets, S = residues("trpcage")
    fsets, fS = PARTITIONS["straddling"](f.n)
    members = [(s, 1, "reference", None, sets, S), (f, 0, "reference", None, fsets, fS), (s, 1, "reference", None, sets, S)]
    ks, bufs = group_and_twins(torch, members, [s.jittered(1), f.pos, s.jittered(2)], ["jitter1", "file", "jitter2"], [2, 1, 2])
    assert [int(k.scalar("energy_only_launches")) + 1 for k in ks] == [5, 3, 5]
    m = bufs[1].result()[1]
    assert (m - np.diag(np.diag(m)) == 0.0).all() and np.diag(m).any()


def test_members_that_cannot_share_run_alone_and_everyone_is_right(gpu_required, systems, five):
    """A fast-mode member with a cutoff and a deterministic member among Reference members: the two run what pair_matrix_device
    runs for them (scalar 19 = 0), the others share; the modes are what they were."""
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    sets, S = residues("trpcage")
    modes = [("reference", None), ("fast", 1.0), ("deterministic", None), ("reference", None)]
    members = [(s, 1, mode, cut, sets, S) for mode, cut in modes]
    ks, _ = group_and_twins(torch, members, [s.jittered(m) for m in range(4)], [f"jitter{m}" for m in range(4)], [2, 0, 0, 2])
    lib = _lib.load()
    assert [lib.agbnp_hip_get_mode(k._h) for k in ks] == [P.HipCalcAGBNPForceKernel.MODES[mode] for mode, _ in modes]


def test_a_group_of_one(gpu_required, systems, five):
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    sets, S = residues("trpcage")
    group_and_twins(torch, [(s, 1, "reference", None, sets, S)], [s.jittered(1)], ["jitter1"], [1])


# ---- 2. the device call adds; the host call overwrites -----------------------------------------------------------------------
def test_the_device_call_adds_and_takes_no_energy_words(gpu_required, systems, five):
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    sets, S = residues("trpcage")
    stream = _stream(torch)
    parts = [(sets, S), (np.arange(s.n) % 3, 3)]
    ks = [_kernel(s, sets=p, num_sets=n) for p, n in parts]
    bufs = [Mats(torch, s.n, n) for _, n in parts]
    geoms = [s.jittered(1), s.jittered(2)]
    for b, g in zip(bufs, geoms):
        b.load(g, 1.0, 2.0)
    pos0 = [b.pos.clone() for b in bufs]
    _mgroup(ks, bufs, stream)
    _mgroup(ks, bufs, stream)
    _mgroup(ks, bufs, stream, energies=False)  # d_energies = NULL is accepted
    assert [k.finish(stream) for k in ks] == [0, 0]
    assert _members(ks) == [2, 2]
    for b, g, tag, p0, (p, n) in zip(bufs, geoms, ("jitter1", "jitter2"), pos0, parts):
        e_ref, ref = reference(s, tag, g, p, n)
        e, m = b.result()
        cells_close(m, 1.0 + 3.0 * ref, 3 * TIGHT, count=3)
        _energy_close(e, 2.0 + 2.0 * e_ref, 2 * TIGHT)
        assert torch.equal(b.pos, p0)


def test_the_host_form_overwrites_and_repeats_a_jumped_member(gpu_required, systems, five):
    s, f = systems("trpcage"), systems("fixture264")
    sets, S = residues("trpcage")
    fsets, fS = PARTITIONS["straddling"](f.n)
    mod3 = np.arange(s.n) % 3
    ks = [_kernel(s, sets=sets), _kernel(f, 0, sets=fsets, num_sets=fS), _kernel(s, sets=mod3)]
    cases = [(s, "jitter1", s.jittered(1), 1, sets, S), (f, "file", f.pos, 0, fsets, fS), (s, "jitter2", s.jittered(2), 1, mod3, 3)]
    energies, matrices = P.pair_matrix_group_host(ks, [c[2] for c in cases])
    for e, m, (x, tag, g, v, p, n) in zip(energies, matrices, cases):
        e_ref, ref = reference(x, tag, g, p, n, version=v)
        cells_close(m, ref)
        _energy_close(e, e_ref)
    moved = s.jittered(3) + np.array([0.1, 0.0, 0.0])  # (the third member jumps: withheld on the device, repeated inside)
    cases = [(s, "jitter4", s.jittered(4), 1, sets, S), (f, "file", f.pos, 0, fsets, fS), (s, "moved3", moved, 1, mod3, 3)]
    energies, matrices = P.pair_matrix_group_host(ks, [c[2] for c in cases])
    for e, m, (x, tag, g, v, p, n) in zip(energies, matrices, cases):
        e_ref, ref = reference(x, tag, g, p, n, version=v)
        cells_close(m, ref)
        _energy_close(e, e_ref)
    assert [k.finish() for k in ks] == [0, 0, 0]


# ---- 3. withheld -------------------------------------------------------------------------------------------------------------
def test_a_jump_is_withheld_for_that_member_only(gpu_required, systems, five):
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    sets, S = residues("trpcage")
    stream = _stream(torch)
    ks = [_kernel(s, sets=sets) for _ in range(3)]
    bufs = [Mats(torch, s.n, S) for _ in ks]
    for b, m in zip(bufs, range(3)):
        b.load(s.jittered(m))
    _mgroup(ks, bufs, stream)
    assert [k.finish(stream) for k in ks] == [0, 0, 0]
    geoms = [s.jittered(10 + m) for m in range(3)]
    geoms[1] = _jumped(s, geoms[1])  # one heavy atom, 0.06 nm
    for b, g in zip(bufs, geoms):
        b.load(g, SENTINEL, SENTINEL)
    _mgroup(ks, bufs, stream)
    assert [k.finish(stream) for k in ks] == [0, 1, 0]
    assert list(ks[1].withheld()) == [0] and int(ks[1].scalar("overflow_kinds")) & JUMP
    e, m = bufs[1].result()
    assert e == SENTINEL and (m == SENTINEL).all()  # bit-unchanged
    for k in (0, 2):
        e_ref, ref = reference(s, f"jitter{10 + k}", geoms[k], sets, S)
        e, m = bufs[k].result()
        cells_close(m - SENTINEL, ref)
        _energy_close(e - SENTINEL, e_ref)
    bufs[1].load(geoms[1])
    _mgroup(ks, bufs, stream)  # the repeat, through the whole group again: the masks lie at the jumped positions now
    assert [k.finish(stream) for k in ks] == [0, 0, 0]
    e_ref, ref = reference(s, "jitter11_jumped", geoms[1], sets, S)
    e, m = bufs[1].result()
    cells_close(m, ref)
    _energy_close(e, e_ref)
    back = s.jittered(12)  # 0.06 nm back: a jump again, not withheld with the hint
    ks[1].expect_jump()
    bufs[1].load(back)
    _mgroup(ks, bufs, stream)
    assert [k.finish(stream) for k in ks] == [0, 0, 0]
    cells_close(bufs[1].result()[1], reference(s, "jitter12", back, sets, S)[1])


# ---- 4. interleaving and launches --------------------------------------------------------------------------------------------
def test_the_four_group_kinds_interleaved_rewrite_no_block(gpu_required, systems, five):
    """execute_group, energy_group, decompose_group and pair_matrix_group of the same three members with fixed position buffers,
    round after round: every result is right; four calls a round meet both parities of every member in the first round, and after
    it no argument block is rewritten; the launch counts and the generation stay; a following execute_device is that of a twin
    that never saw a matrix call."""
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    sets, S = residues("trpcage")
    oracle = Oracle(*s.params(), version=1)
    stream = _stream(torch)
    dev = torch.device("cuda:0")
    ks = [_kernel(s, sets=sets) for _ in range(3)]
    twin = _kernel(s)
    for k in ks + [twin]:
        k.execute(s.pos, np.zeros((s.n, 3)))
    state = [(k.generation(), int(k.scalar("launches")), int(k.scalar("energy_only_launches"))) for k in ks]
    assert [st[1:] for st in state] == [(5, 4)] * 3
    bufs = [Buffers(torch, s.n) for _ in ks]
    planes = [torch.zeros((4, s.n), dtype=torch.float64, device=dev) for _ in ks]
    mats = [torch.zeros((S, S), dtype=torch.float64, device=dev) for _ in ks]
    pos_ptrs = [b.pos.data_ptr() for b in bufs]
    ene_ptrs = [b.ene.data_ptr() for b in bufs]
    settled = None
    step = 0
    for rnd in range(3):
        for what in "FEDM":
            geoms = [s.jittered(40 * m + step) for m in range(3)]
            for b, g, p, x in zip(bufs, geoms, planes, mats):
                b.load(g, SENTINEL if what != "F" else 0.0)
                p.zero_()
                x.zero_()
            if what == "F":
                _fgroup(ks, bufs, stream)
            elif what == "E":
                P.energy_group(ks, pos_ptrs, ene_ptrs, stream)
            elif what == "D":
                P.decompose_group(ks, pos_ptrs, [p.data_ptr() for p in planes], ene_ptrs, stream)
            else:
                P.pair_matrix_group(ks, pos_ptrs, [x.data_ptr() for x in mats], ene_ptrs, stream)
            assert [k.finish(stream) for k in ks] == [0, 0, 0]
            assert _kinds(ks) == [dict(F=0, E=1, D=3, M=4)[what]] * 3 and _members(ks) == [3, 3, 3]
            for m, (b, g, p, x) in enumerate(zip(bufs, geoms, planes, mats)):
                e, f = b.result()
                eo, fo = oracle.execute(g)
                if what == "F":
                    _close(e, f, eo, fo)
                else:
                    assert (f == SENTINEL).all(), "a force buffer was written"
                    _energy_close(e, eo)
                if what == "M":
                    cells_close(x.cpu().numpy(), reference(s, f"jitter{40 * m + step}", g, sets, S)[1])
                else:
                    assert not x.any().item()
                if what == "D":
                    assert abs(p.sum().item() - eo) < TIGHT * max(1.0, 1e-3 * abs(eo))
                else:
                    assert not p.any().item()
            step += 1
        writes = [int(k.scalar("group_block_writes")) for k in ks]
        print("round", rnd, "group_block_writes", writes)
        if rnd == 0:
            settled = writes
        assert writes == settled, "a steady run of mixed group calls rewrote an argument block"
    assert settled == [2, 2, 2]  # (one write per parity, whichever kind of call met it first)
    assert [(k.generation(), int(k.scalar("launches")), int(k.scalar("energy_only_launches"))) for k in ks] == state
    last = s.jittered(step)
    out = []
    for k in (ks[0], twin):
        b = Buffers(torch, s.n)
        b.load(last)
        k.execute_device(*b.ptrs(), stream)
        assert k.finish(stream) == 0 and int(k.scalar("last_evaluation_kind")) == 0
        out.append(b.result())
    assert abs(out[0][0] - out[1][0]) < SAME and np.abs(out[0][1] - out[1][1]).max() < SAME


# ---- 5. refusals: argument checks that return before any launch --------------------------------------------------------------
def test_the_refusals(gpu_required, systems, five):
    torch = pytest.importorskip("torch")
    lib = _lib.load()
    s = systems("trpcage")
    sets, S = residues("trpcage")
    stream = _stream(torch)
    ks = [_kernel(s, sets=sets) for _ in range(2)]
    bare = _kernel(s)
    bufs = [Mats(torch, s.n, S) for _ in ks]
    for b, m in zip(bufs, range(2)):
        b.load(s.jittered(m))
    _mgroup(ks, bufs, stream)
    assert [k.finish(stream) for k in ks] == [0, 0]
    for b, m in zip(bufs, range(2)):
        b.load(s.jittered(m), SENTINEL, SENTINEL)
    pos, mats, ene = ([b.pos.data_ptr() for b in bufs], [b.matrix.data_ptr() for b in bufs], [b.ene.data_ptr() for b in bufs])
    arr2 = C.c_void_p * 2

    def raw(handles, p, m, e):
        """The library itself, past the wrapper's own checks."""
        return lib.agbnp_hip_pair_matrix_group(arr2(*handles), 2, arr2(*p), arr2(*m), arr2(*e) if e else None, C.c_void_p(stream))
    # a member without a partition: the wrapper refuses, and so does the library itself
    with pytest.raises(P.OpenMMException, match="no partition has been set"):
        P.pair_matrix_group([ks[0], bare], pos, mats, ene, stream)
    assert raw([ks[0]._h, bare._h], pos, mats, ene) == _lib.ERR_INVALID_ARGUMENT
    assert "no partition has been set" in _lib.last_error(ks[0]._h)
    # 0 and 17 members
    with pytest.raises(P.OpenMMException, match="1 to 16"):
        P.pair_matrix_group([], [], [], None, stream)
    with pytest.raises(P.OpenMMException, match="1 to 16"):
        P.pair_matrix_group([ks[0]] * 17, pos[:1] * 17, mats[:1] * 17, None, stream)
    arr = C.c_void_p * 17
    handles, p17 = arr(*[ks[0]._h] * 17), arr(*[pos[0]] * 17)
    assert lib.agbnp_hip_pair_matrix_group(handles, 17, p17, p17, None, None) == _lib.ERR_INVALID_ARGUMENT
    assert "1 to 16" in _lib.last_error(ks[0]._h)
    assert lib.agbnp_hip_pair_matrix_group(handles, 0, p17, p17, None, None) == _lib.ERR_INVALID_ARGUMENT
    # a context passed twice
    with pytest.raises(P.OpenMMException, match="twice"):
        P.pair_matrix_group([ks[0], ks[0]], pos, mats, ene, stream)
    # matrix spans [S S] that overlap by one word, and an energy word inside a matrix: another member's, and its own
    last = 8 * (S * S - 1)
    for m2, e2 in (([mats[0], mats[0] + last], ene), (mats, [mats[1] + 8, ene[1]]), (mats, [ene[0], mats[1] + last])):
        with pytest.raises(P.OpenMMException, match="matrices of two members overlap"):
            P.pair_matrix_group(ks, pos, m2, e2, stream)
        assert raw([k._h for k in ks], pos, m2, e2) == _lib.ERR_INVALID_ARGUMENT
        assert "matrices of two members overlap" in _lib.last_error(ks[0]._h)
    with pytest.raises(P.OpenMMException, match="energy words of two members overlap"):
        P.pair_matrix_group(ks, pos, mats, [ene[0], ene[0]], stream)
    with pytest.raises(P.OpenMMException, match="null pointer"):
        P.pair_matrix_group(ks, pos, [mats[0], 0], ene, stream)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        bufs[0].ene.fill_(1.0)
        with pytest.raises(P.OpenMMException, match="captur"):
            _mgroup(ks, bufs, torch.cuda.current_stream().cuda_stream)
    g.replay()
    torch.cuda.synchronize()
    # nothing was launched, no member changed: no evaluation in any log, the buffers as they were, and the group works
    assert [k.wait_verdict() for k in ks] == [(0, 0), (0, 0)]  # (evaluations enqueued since the last finish: none)
    assert [k.finish(stream) for k in ks + [bare]] == [0, 0, 0]
    assert bufs[0].ene.item() == 1.0 and bufs[1].ene.item() == SENTINEL
    assert all((b.matrix == SENTINEL).all().item() for b in bufs)
    for b, m in zip(bufs, range(2)):
        b.load(s.jittered(m))
    _mgroup(ks, bufs, stream)
    assert [k.finish(stream) for k in ks] == [0, 0]
    for b, m in zip(bufs, range(2)):
        cells_close(b.result()[1], reference(s, f"jitter{m}", s.jittered(m), sets, S)[1])


# ---- 6. the C++ mirror -------------------------------------------------------------------------------------------------------
def test_cxx_mirror(gpu_required, systems, five, tmp_path):
    """tests/cxx/TestHipPairMatrixGroup.cpp through cpp/AGBNPForce.h."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(root, "openmm_agbnp_plugin_amd")
    exe = str(tmp_path / "TestHipPairMatrixGroup")
    subprocess.run(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    os.path.join(root, "tests", "cxx", "TestHipPairMatrixGroup.cpp"), "-o", exe, os.path.join(libdir, "libagbnp_hip.so"),
                    "-L/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    x = systems("trpcage")
    sets, _ = residues("trpcage")
    path = tmp_path / "trpcage.txt"
    r, g, a, q, h = x.params()
    np.savetxt(path, np.column_stack([r, g, a, q, np.asarray(h, dtype=float), x.pos, sets.astype(float)]), fmt="%.17g")
    out = subprocess.run([exe, str(path), "16"], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
