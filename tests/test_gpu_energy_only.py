"""GPU box: energy-only evaluations (include/agbnp_hip.h: agbnp_hip_energy_host / _device / _openmm) -- what
OpenMM asks for with includeForces = false.  The energy of the matching full evaluation, no force written anywhere, the same
overflow log, and a context left exactly as a full evaluation leaves it, so that the two kinds interleave in any order."""
import numpy as np
import pytest

import openmm_agbnp_plugin_amd as P
from oracle import Oracle
from tests.gpu_helpers import SAME
from tests.gpu_helpers import close as _close
from tests.gpu_helpers import energy_close as _energy_close
from tests.gpu_helpers import five  # noqa: F401

pytestmark = pytest.mark.gpu
SENTINEL = 0x5A5A_1234_A5A5_4321
FULL_KERNELS = {"k_tree_cavity", "k_born_rows", "k_gb_tiles", "k_dborn_rows", "k_tree_pseudo"}


def _kernel(s, version=1, mode="reference", cutoff=None):
    k = P.HipCalcAGBNPForceKernel(device=0, mode=mode)
    force = P.AGBNPForce.from_arrays(*s.params(), version=version)
    if cutoff is not None:
        force.setNonbondedMethod(P.AGBNPForce.CutoffNonPeriodic)
        force.setCutoffDistance(cutoff)
    k.initialize(force)
    return k


@pytest.mark.parametrize("version,name", [(1, "trpcage"), (1, "1dwc"), (1, "2clr"), (1, "fixture264"), (0, "trpcage"), (0, "fixture264")])
def test_energy_only_matches_the_oracle_and_the_full_evaluation(gpu_required, systems, five, version, name):
    """Unrelated geometries through the host entry point (jumps: withheld, repeated inside): the oracle's energy, and the
    energy of a full evaluation at the same positions."""
    s = systems(name)
    k = _kernel(s, version)
    oracle = Oracle(*s.params(), version=version)
    centre = s.pos.mean(axis=0)
    for pos in (s.pos, s.jittered(1), s.jittered(2, sigma=0.02), centre + 0.97 * (s.pos - centre), s.pos):
        e_only = k.energy(pos)
        f = np.zeros((s.n, 3))
        e_full = k.execute(pos, f)
        eo, fo = oracle.execute(pos)
        _energy_close(e_only, eo)
        _close(e_full, f, eo, fo)
        assert abs(e_only - e_full) < SAME, f"energy-only {e_only!r} vs full {e_full!r}"
    in_mode = int(k.scalar("launches")) == (5 if version == 1 else 2)  # (capacity variant 4 ends the five-launch mode: the fallback)
    assert int(k.scalar("energy_only_launches")) == ((4 if version == 1 else 2) if in_mode else 0)


def _context_arrays(torch, dev, pos, order, padded, precision):
    """posq (+ correction) in a shuffled, padded context order, and the positions the engine sees."""
    n = len(order)
    host = np.zeros((padded, 4))
    host[:n, :3] = pos[order]
    if precision == "double":
        return torch.tensor(host, dtype=torch.float64, device=dev), None, pos
    hi = host.astype(np.float32)
    lo = (host - hi.astype(np.float64)).astype(np.float32)
    seen = np.zeros((n, 3))
    back = hi.astype(np.float64) + (lo.astype(np.float64) if precision == "mixed" else 0.0)
    seen[order] = back[:n, :3]
    return torch.tensor(hi, device=dev), (torch.tensor(lo, device=dev) if precision == "mixed" else None), seen


@pytest.mark.parametrize("precision", ["double", "mixed", "single"])
def test_energy_openmm_writes_no_force(gpu_required, systems, five, precision):
    """The OpenMM entry point in the three precisions, atoms shuffled and padded: the context's fixed-point force planes keep a
    sentinel pattern bit for bit, the energy reaches the given slot and equals the full evaluation's."""
    torch = pytest.importorskip("torch")
    s = systems("1dwc")
    n, padded = s.n, (s.n + 31) // 32 * 32
    k = _kernel(s)
    oracle = Oracle(*s.params(), version=1)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    order = np.random.default_rng(5).permutation(n).astype(np.int32)
    index = torch.tensor(np.concatenate([order, np.arange(n, padded, dtype=np.int32)]), device=dev)
    dbl = precision != "single"
    edt = torch.float64 if dbl else torch.float32
    sentinel = torch.full((3 * padded,), SENTINEL, dtype=torch.int64, device=dev)
    fixed = sentinel.clone()
    scratch = torch.zeros(3 * padded, dtype=torch.int64, device=dev)
    keep = []
    for step in range(4):
        posq, corr, seen = _context_arrays(torch, dev, s.jittered(step), order, padded, precision)
        keep.append((posq, corr))
        e_full = torch.zeros(8, dtype=edt, device=dev)
        e_only = torch.zeros(8, dtype=edt, device=dev)
        cp = corr.data_ptr() if corr is not None else 0
        k.execute_openmm(posq.data_ptr(), precision == "double", cp, index.data_ptr(), padded, scratch.data_ptr(), e_full.data_ptr(), dbl, 2, stream)
        k.energy_openmm(posq.data_ptr(), precision == "double", cp, index.data_ptr(), padded, e_only.data_ptr(), dbl, 5, stream)
        assert k.finish(stream) == 0, (list(k.withheld()), int(k.scalar("overflow_kinds")))
        torch.cuda.synchronize()
        assert torch.equal(fixed, sentinel)
        ef, eo_ = e_full.cpu().numpy().astype(np.float64), e_only.cpu().numpy().astype(np.float64)
        assert np.count_nonzero(eo_) == 1 and eo_[5] != 0.0
        if dbl:
            assert abs(eo_[5] - ef[2]) < SAME
            _energy_close(eo_[5], oracle.execute(seen)[0])
        else:
            assert abs(eo_[5] - ef[2]) <= 1e-6 * abs(ef[2])
    assert int(k.scalar("energy_only_launches")) == 4


@pytest.mark.parametrize("version,name", [(1, "1dwc"), (0, "trpcage")])
def test_energy_only_launch_shape(gpu_required, systems, five, version, name):
    """A settled context: energy-only evaluations launch neither the chain-rule nor the pseudo-volume launch -- scalar 18 of
    them per evaluation -- and the same context's full evaluations still launch the five kernels (version 0: two)."""
    s = systems(name)
    k = _kernel(s, version)
    f = np.zeros((s.n, 3))
    for step in range(4):
        k.execute(s.jittered(step), f)
    k.set_profiling(True)
    evals = 4
    for step in range(4, 4 + evals):
        k.energy(s.jittered(step))
    times = {n: v for n, v in k.kernel_times().items() if v[1] > 0}
    k.set_profiling(False)
    assert "k_tree_pseudo" not in times and "k_dborn_rows" not in times and "k_prep" not in times, times
    launches = sum(v[1] for v in times.values())
    expect = int(k.scalar("energy_only_launches"))
    assert expect == (4 if version == 1 else 2)
    assert launches == expect * evals, times
    k.set_profiling(True)
    for step in range(8, 8 + evals):
        k.execute(s.jittered(step), f)
    times = {n for n, v in k.kernel_times().items() if v[1] > 0}
    k.set_profiling(False)
    assert times == (FULL_KERNELS if version == 1 else {"k_tree_cavity", "k_outputs"}), times


@pytest.mark.parametrize("name,every", [("trpcage", 1), ("1dwc", 10)])
def test_interleaved_walk_and_a_jump(gpu_required, systems, five, name, every):
    """Full and energy-only evaluations alternate along a queued cumulative random walk that crosses several replans of the
    forest packing and renews the neighbour masks: each one is the oracle's.  Then a jump inside an energy-only evaluation:
    withheld alone, the repeat is right, the full evaluation behind it is exact; the host entry point repeats by itself."""
    torch = pytest.importorskip("torch")
    s = systems(name)
    k = _kernel(s)
    oracle = Oracle(*s.params(), version=1)
    rng = np.random.default_rng(7)
    steps = 150
    walk = s.pos + np.cumsum(rng.normal(0.0, 0.0015, (steps,) + s.pos.shape), axis=0)
    dev = torch.device("cuda:0")
    pos = torch.tensor(walk, dtype=torch.float64, device=dev).contiguous()
    frc = torch.zeros((steps, s.n, 3), dtype=torch.float64, device=dev)
    ene = torch.zeros((steps,), dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    f0 = np.zeros((s.n, 3))
    k.execute(s.pos, f0)  # (settles the capacity variant and the first masks)
    plans0 = int(k.scalar("pack_plans"))
    for i in range(steps):
        if i % 2 == 0:
            k.execute_device(pos[i].data_ptr(), frc[i].data_ptr(), ene[i:i + 1].data_ptr(), stream)
        else:
            k.energy_device(pos[i].data_ptr(), ene[i:i + 1].data_ptr(), stream)
    assert k.finish(stream) == 0, (k.withheld(), int(k.scalar("overflow_kinds")))
    assert int(k.scalar("pack_plans")) - plans0 >= 3  # (a replan every 16 evaluations)
    assert float(np.linalg.norm(walk[-1] - s.pos, axis=1).max()) > 0.03  # (the walk did leave the first masks' skin)
    e_got, f_got = ene.cpu().numpy(), frc.cpu().numpy()
    assert not f_got[1::2].any()  # (nothing is written for the energy-only ones: their force rows stayed zero)
    for i in range(0, steps, every):
        eo, fo = oracle.execute(walk[i])
        if i % 2 == 0:
            _close(e_got[i], f_got[i], eo, fo)
        else:
            _energy_close(e_got[i], eo)
        if every > 1:  # (and its energy-only neighbour)
            eo1, _ = oracle.execute(walk[i + 1])
            _energy_close(e_got[i + 1], eo1)
    # a jump (every atom ~0.05 nm away at once) inside an energy-only evaluation in the middle of a queue
    last = walk[-1]
    jump = last + np.random.default_rng(3).normal(0.0, 0.03, s.pos.shape)
    geoms = [last + 0.001, jump, jump + 0.001]
    gpos = torch.tensor(np.stack(geoms), dtype=torch.float64, device=dev).contiguous()
    gfrc = torch.zeros((3, s.n, 3), dtype=torch.float64, device=dev)
    gene = torch.zeros((3,), dtype=torch.float64, device=dev)
    k.execute_device(gpos[0].data_ptr(), gfrc[0].data_ptr(), gene[0:1].data_ptr(), stream)
    k.energy_device(gpos[1].data_ptr(), gene[1:2].data_ptr(), stream)
    k.execute_device(gpos[2].data_ptr(), gfrc[2].data_ptr(), gene[2:3].data_ptr(), stream)
    assert k.finish(stream) == 1 and list(k.withheld()) == [1]
    assert int(k.scalar("overflow_kinds")) & 16
    assert gene[1].item() == 0.0
    k.energy_device(gpos[1].data_ptr(), gene[1:2].data_ptr(), stream)  # the repeat
    assert k.finish(stream) == 0
    e_got, f_got = gene.cpu().numpy(), gfrc.cpu().numpy()
    want = [oracle.execute(g) for g in geoms]
    _close(e_got[0], f_got[0], *want[0])
    _energy_close(e_got[1], want[1][0])
    _close(e_got[2], f_got[2], *want[2])
    # the host entry point across another jump repeats by itself
    jump2 = geoms[2] + np.random.default_rng(4).normal(0.0, 0.03, s.pos.shape)
    _energy_close(k.energy(jump2), oracle.execute(jump2)[0])


def test_twenty_queued_energy_only_evaluations(gpu_required, systems, five):
    """Twenty energy-only evaluations into twenty slots, no finish in between: each slot is the oracle's, nothing withheld."""
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    k = _kernel(s)
    oracle = Oracle(*s.params(), version=1)
    f0 = np.zeros((s.n, 3))
    k.execute(s.pos, f0)
    rng = np.random.default_rng(21)
    walk = s.pos + np.cumsum(rng.normal(0.0, 0.001, (20,) + s.pos.shape), axis=0)
    dev = torch.device("cuda:0")
    pos = torch.tensor(walk, dtype=torch.float64, device=dev).contiguous()
    ene = torch.zeros((20,), dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    for i in range(20):
        k.energy_device(pos[i].data_ptr(), ene[i:i + 1].data_ptr(), stream)
    assert k.finish(stream) == 0, (k.withheld(), int(k.scalar("overflow_kinds")))
    got = ene.cpu().numpy()
    for i in range(20):
        _energy_close(got[i], oracle.execute(walk[i])[0])


@pytest.mark.parametrize("flavour", ["deterministic", "fast", "fast+single", "rows0", "five0", "captured"])
def test_the_fallback_configurations(gpu_required, systems, five, monkeypatch, flavour):
    """Where the energy-only launches do not apply, the evaluation runs as a full one with its forces sent to the context's own
    buffer: the energy of that configuration's full evaluation (bit-identical in the deterministic mode), scalar 18 says 0,
    and no force reaches the caller (the OpenMM entry point's sentinel planes stay as they were)."""
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    if flavour == "rows0":
        monkeypatch.setenv("AGBNP_HIP_ROWS", "0")
    if flavour == "five0":
        monkeypatch.setenv("AGBNP_HIP_FIVE_LAUNCHES", "0")
    mode = flavour if flavour in ("deterministic", "fast", "fast+single") else "reference"
    k = _kernel(s, mode=mode, cutoff=1.0 if mode.startswith("fast") else None)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    f0 = np.zeros((s.n, 3))
    k.execute(s.pos, f0)
    if flavour == "captured":
        cpos = torch.tensor(s.jittered(1), dtype=torch.float64, device=dev).contiguous()
        cfrc = torch.zeros((s.n, 3), dtype=torch.float64, device=dev)
        cene = torch.zeros((1,), dtype=torch.float64, device=dev)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            cfrc.zero_()
            cene.zero_()
            k.execute_device(cpos.data_ptr(), cfrc.data_ptr(), cene.data_ptr(), torch.cuda.current_stream().cuda_stream)
        g.replay()
        torch.cuda.synchronize()
        assert k.finish(stream) == 0
    assert int(k.scalar("energy_only_launches")) == 0
    tol = 1e-6 if flavour == "fast+single" else SAME
    for step in (2, 3):
        geom = s.jittered(step)
        pos = torch.tensor(geom, dtype=torch.float64, device=dev).contiguous()
        frc = torch.zeros((s.n, 3), dtype=torch.float64, device=dev)
        e_full = torch.zeros((1,), dtype=torch.float64, device=dev)
        e_only = torch.zeros((1,), dtype=torch.float64, device=dev)
        k.execute_device(pos.data_ptr(), frc.data_ptr(), e_full.data_ptr(), stream)
        k.energy_device(pos.data_ptr(), e_only.data_ptr(), stream)
        assert k.finish(stream) == 0
        a, b = e_full.item(), e_only.item()
        if flavour == "deterministic":
            assert a == b, (a, b)
        else:
            assert abs(a - b) < tol, (a, b)
    # the OpenMM entry point: nothing reaches the context's fixed-point planes
    n, padded = s.n, (s.n + 31) // 32 * 32
    index = torch.tensor(np.concatenate([np.arange(n - 1, -1, -1, dtype=np.int32), np.arange(n, padded, dtype=np.int32)]), device=dev)
    order = index.cpu().numpy()[:n]
    posq, _, _ = _context_arrays(torch, dev, s.jittered(3), order, padded, "double")
    sentinel = torch.full((3 * padded,), SENTINEL, dtype=torch.int64, device=dev)
    fixed = sentinel.clone()
    ebuf = torch.zeros(4, dtype=torch.float64, device=dev)
    eref = torch.zeros(4, dtype=torch.float64, device=dev)
    scratch = torch.zeros(3 * padded, dtype=torch.int64, device=dev)
    k.execute_openmm(posq.data_ptr(), True, 0, index.data_ptr(), padded, scratch.data_ptr(), eref.data_ptr(), True, 1, stream)
    k.energy_openmm(posq.data_ptr(), True, 0, index.data_ptr(), padded, ebuf.data_ptr(), True, 1, stream)
    k.energy_openmm(posq.data_ptr(), True, 0, index.data_ptr(), padded, ebuf.data_ptr(), True, 2, stream)
    assert k.finish(stream) == 0, (list(k.withheld()), int(k.scalar("overflow_kinds")))
    torch.cuda.synchronize()
    assert torch.equal(fixed, sentinel)
    got, ref = ebuf.cpu().numpy(), eref.cpu().numpy()
    assert got[0] == 0.0 and got[3] == 0.0 and ref[1] != 0.0
    for slot in (1, 2):
        assert (got[slot] == ref[1]) if flavour == "deterministic" else abs(got[slot] - ref[1]) < tol, (slot, got, ref)
    assert int(k.scalar("energy_only_launches")) == 0


def test_energy_device_refuses_a_stream_capture(gpu_required, systems, five):
    """Energy-only graphs are not supported: inside a capture the call fails with INVALID_ARGUMENT, launches nothing, and the
    capture ends cleanly and replays."""
    torch = pytest.importorskip("torch")
    s = systems("trpcage")
    k = _kernel(s)
    oracle = Oracle(*s.params(), version=1)
    f0 = np.zeros((s.n, 3))
    k.execute(s.pos, f0)
    dev = torch.device("cuda:0")
    pos = torch.tensor(s.jittered(1), dtype=torch.float64, device=dev).contiguous()
    ene = torch.zeros((1,), dtype=torch.float64, device=dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ene.fill_(1.0)
        with pytest.raises(P.OpenMMException, match="captur"):
            k.energy_device(pos.data_ptr(), ene.data_ptr(), torch.cuda.current_stream().cuda_stream)
    ene.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert ene.item() == 1.0
    # the context goes on as before: still the energy-only launches, still the oracle's energy
    assert int(k.scalar("energy_only_launches")) == 4
    _energy_close(k.energy(s.jittered(1)), oracle.execute(s.jittered(1))[0])


def test_getenergy_honours_the_force_group(gpu_required, systems, five):
    s = systems("trpcage")
    force = P.AGBNPForce.from_arrays(*s.params(), version=1)
    ctx = P.AGBNPContext(force, device=0)
    ctx.setPositions(s.pos)
    e, _ = ctx.getState()
    assert abs(ctx.getEnergy() - e) < SAME
    force.setForceGroup(3)
    assert ctx.getEnergy(groups=1 << 2) == 0.0
