"""GPU box: perturbation groups (include/agbnp_hip.h: agbnp_hip_perturbed_energies_group / _host).  Every member
of a group must get what its own agbnp_hip_perturbed_energies_device would give it, over its own sets: every E_m is that of a
twin context evaluated alone (SAME = 1e-9, scaled) and the oracle's with set m (TIGHT), its verdict and its overflow log are its
own, and the call is refused as a whole -- nothing launched -- when a member has no sets or stands twice."""
import numpy as np
import pytest

import openmm_agbnp_plugin_amd as P
from tests.gpu_helpers import SAME, energy_close
from tests.gpu_helpers import five_groups as five  # noqa: F401
from tests.perturbation_restatement import ladder
from tests.test_gpu_perturbation import _kernel, all_close, reference, three_sets

pytestmark = pytest.mark.gpu


class Words:
    """Device positions, energies under the sets and own energy of one member."""

    def __init__(self, torch, n, m, fill=0.0):
        dev = torch.device("cuda:0")
        self.torch = torch
        self.pos = torch.zeros((n, 3), dtype=torch.float64, device=dev)
        self.out = torch.full((m,), fill, dtype=torch.float64, device=dev)
        self.own = torch.full((1,), fill, dtype=torch.float64, device=dev)

    def load(self, geom, fill=0.0):
        self.pos.copy_(self.torch.tensor(np.asarray(geom), dtype=self.torch.float64))
        self.out.fill_(fill)
        self.own.fill_(fill)


def _pgroup(kernels, bufs, stream, own=True):
    P.perturbed_energies_group(kernels, [b.pos.data_ptr() for b in bufs], [b.out.data_ptr() for b in bufs],
                               [b.own.data_ptr() for b in bufs] if own else None, stream)


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


def the_three_members(systems):
    """trpcage version 1 with four sets, fixture264 version 1 with two, trpcage version 0 with three: (system, version, sets, tag)."""
    t, f = systems("trpcage"), systems("fixture264")
    return [(t, 1, ladder(t.params(), 16)[:4], "ladder"), (f, 1, three_sets(f)[:2], "file"), (t, 0, three_sets(t), "file")]


def member_reference(s, v, sets, tag):
    if tag == "ladder":  # (shared with tests/test_gpu_perturbation.py: the sixteen rungs once)
        return reference(s, tag, s.pos, ladder(s.params(), 16), version=v)[:len(sets)]
    return reference(s, tag, s.pos, three_sets(s), version=v)[:len(sets)]


def test_every_member_equals_its_own_single_call(gpu_required, systems, five):
    torch = pytest.importorskip("torch")
    stream = _stream(torch)
    members = the_three_members(systems)
    ks = [_kernel(s, version=v, sets=sets) for s, v, sets, _ in members]
    twins = [_kernel(s, version=v, sets=sets) for s, v, sets, _ in members]
    bufs = [Words(torch, s.n, len(sets)) for s, _, sets, _ in members]
    tb = [Words(torch, s.n, len(sets)) for s, _, sets, _ in members]
    for attempt in range(4):  # (a first evaluation withheld for a capacity climb is repeated the way a caller repeats)
        for (s, _, _, _), b, t in zip(members, bufs, tb):
            b.load(s.pos)
            t.load(s.pos)
        _pgroup(ks, bufs, stream)
        for tw, t in zip(twins, tb):
            tw.perturbed_energies_device(t.pos.data_ptr(), t.out.data_ptr(), t.own.data_ptr(), stream)
        withheld = [k.finish(stream) for k in ks]
        assert [k.finish(stream) for k in twins] == withheld
        if not any(withheld):
            break
    assert not any(withheld)
    assert [int(k.scalar("last_evaluation_kind")) for k in ks] == [5, 5, 5]
    assert [int(k.scalar("group_members")) for k in ks] == [2, 2, 1]  # the version-0 member forms a launch set of its own
    assert [int(k.scalar("energy_only_launches")) + 1 for k in ks] == [5, 5, 3]  # the energy-only group's launches plus ONE
    for (s, v, sets, tag), b, t in zip(members, bufs, tb):
        e, te = b.out.cpu().numpy(), t.out.cpu().numpy()
        all_close(f"{s.name} v{v} against its twin", e, te, SAME)
        energy_close(b.own.item(), t.own.item(), SAME)
        all_close(f"{s.name} v{v}", e, member_reference(s, v, sets, tag))
    # the host form: the same numbers, OVERWRITTEN
    own, energies = P.perturbed_energies_group_host(ks, [m[0].pos for m in members])
    for (s, v, sets, tag), b, o, e in zip(members, bufs, own, energies):
        all_close(f"{s.name} v{v} host form", e, b.out.cpu().numpy(), SAME)
        energy_close(o, b.own.item(), SAME)


def test_a_withheld_member_does_not_touch_the_others(gpu_required, systems, five):
    torch = pytest.importorskip("torch")
    stream = _stream(torch)
    s = systems("trpcage")
    sets = three_sets(s)
    ks = [_kernel(s, sets=sets) for _ in range(3)]
    bufs = [Words(torch, s.n, 3) for _ in ks]
    for k in ks:
        k.execute(s.pos, np.zeros((s.n, 3)))
    heavy = np.flatnonzero(s.ishydrogen == 0)
    moved = s.pos.copy()
    moved[heavy[len(heavy) // 2], 0] += 0.06  # beyond the masks' skin: member 1 jumps without a hint
    for b, g in zip(bufs, (s.pos, moved, s.pos)):
        b.load(g, 1.0)
    _pgroup(ks, bufs, stream)
    assert [k.finish(stream) for k in ks] == [0, 1, 0]
    assert list(ks[1].withheld()) == [0]
    torch.cuda.synchronize()
    assert (bufs[1].out == 1.0).all().item() and bufs[1].own.item() == 1.0  # nothing was added to either output
    ref = reference(s, "file", s.pos, sets)
    for b in (bufs[0], bufs[2]):
        all_close("trpcage beside a withheld member", b.out.cpu().numpy(), 1.0 + ref)
        energy_close(b.own.item(), 1.0 + ref[0])
    # no own-energy words at all is accepted (the masks of the withheld member lie at `moved`: its host entry jumps back first)
    ks[1].execute(s.pos, np.zeros((s.n, 3)))
    for b in bufs:
        b.load(s.pos)
    _pgroup(ks, bufs, stream, own=False)
    assert [k.finish(stream) for k in ks] == [0, 0, 0]
    for b in bufs:
        all_close("trpcage without own words", b.out.cpu().numpy(), ref)
        assert b.own.item() == 0.0


def test_a_member_without_sets_or_a_duplicate_refuses_the_whole_call(gpu_required, systems, five):
    torch = pytest.importorskip("torch")
    stream = _stream(torch)
    s = systems("trpcage")
    sets = three_sets(s)
    with_sets, without = _kernel(s, sets=sets), _kernel(s)
    for k in (with_sets, without):
        k.execute(s.pos, np.zeros((s.n, 3)))
    bufs = [Words(torch, s.n, 3, 1.0) for _ in range(2)]
    for b in bufs:
        b.load(s.pos, 1.0)
    state = [(k.generation(), int(k.scalar("launches")), int(k.scalar("energy_only_launches"))) for k in (with_sets, without)]
    with pytest.raises(P.OpenMMException, match="no parameter sets have been set"):
        _pgroup([with_sets, without], bufs, stream)
    # ... and by the library itself, past the wrapper's own check
    without._num_parameter_sets = 3
    with pytest.raises(P.OpenMMException, match="member 1: no parameter sets have been set"):
        _pgroup([with_sets, without], bufs, stream)
    with pytest.raises(P.OpenMMException, match="twice"):
        _pgroup([with_sets, with_sets], bufs, stream)
    with pytest.raises(P.OpenMMException):
        P.perturbed_energies_group_host([with_sets, without], [s.pos, s.pos])
    assert [k.finish(stream) for k in (with_sets, without)] == [0, 0]
    torch.cuda.synchronize()
    for b in bufs:
        assert (b.out == 1.0).all().item() and b.own.item() == 1.0  # nothing was launched
    assert [(k.generation(), int(k.scalar("launches")), int(k.scalar("energy_only_launches"))) for k in (with_sets, without)] == state
    own, energies = with_sets.perturbed_energies(s.pos)  # (the members go on)
    all_close("trpcage", energies, reference(s, "file", s.pos, sets))
