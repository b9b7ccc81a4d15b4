"""GPU box: the six kernels of csrc/md_kernels.hip alone, one launch at a time, against the CPU restatement of
tests/md_restatement.py (long double; checked against itself by tests/test_md_restatement.py).  No engine and no `systems`
fixture: the state is synthetic, and the evaluation between two launches is a harmonic stand-in made on the host from the
positions read back, so kernel and restatement see bit-identical inputs.  Before and after every launch the whole state is read
back; the "before" goes to the restatement and the "after" is compared with its prediction word by word:

  x, v             1e-11 nm, 1e-9 nm/ps (the bounds of tests/test_md_examples.py and tests/test_gpu_replica_md.py)
  f                -k (x_device - x0) to 1e-9 relative elementwise (as test_the_front_half_is_its_numpy_restatement)
  energies         every tether partial, `last` and every written log slot by tests.gpu_helpers.energy_close (the project's 1e-7)
  everything else  bit for bit: the step words, the energy word, acc, done, the constants, and every sentinel where nothing may
                   be written (acc[r][1], log slots other than the step's or beyond the capacity, the logs' padding tail, the
                   partial buffer not being written, `last` in front of the first back half)

The measured maxima are printed per case."""
import ctypes as C
import types

import numpy as np
import pytest

from tests import md_restatement as mr
from tests.gpu_helpers import TIGHT, energy_close
from tests.md_kernel_harness import CASES, Device, Part, _bits, _note, _same, _up, altered, gpu, record_buffer, split_records  # noqa: F401

pytestmark = pytest.mark.gpu

LANGEVIN, VERLET = mr.LANGEVIN, mr.VERLET
_ENERGIES = ("last", "log_pe", "log_ke")
_EXACT = ("x0", "hdt_m", "mass", "kT", "seeds", "step", "energy", "acc", "done")


def _energies_close(what, before, after, want, worst):
    """Where the prediction differs from the state before, the word was to be written: energy_close there, bits kept elsewhere."""
    written = _bits(want) != _bits(before)
    assert np.array_equal(_bits(after)[~written], _bits(before)[~written]), f"{what}: a word that was not to be written changed"
    for e, eo in zip(after[written], want[written]):
        assert np.isfinite(e) and np.isfinite(eo), f"{what}: {e} for {eo}"
        _note(worst, "dE", abs(e - eo))
        _note(worst, "dE/allowed", abs(e - eo) / (TIGHT * max(1.0, abs(eo) * 1e-3)))
        energy_close(e, eo)
    return written


def compare(what, before, after, want, moved, worst):
    """The state after one launch against the restatement's prediction.  `moved`: which of x, v, f the launch rewrites."""
    for key, tol in (("x", 1e-11), ("v", 1e-9)):
        if key in moved:
            d = np.abs(after[key] - want[key]).max()
            _note(worst, "d" + key, d)
            assert d < tol, f"{what}: {key} differs by {d:.3e}"
        else:
            assert _same(after[key], before[key]), f"{what}: {key} changed"
    if "f" in moved:
        tether = -before["k"] * (after["x"] - after["x0"][None])
        with np.errstate(invalid="ignore", divide="ignore"):
            rel = np.where(tether != 0.0, np.abs(after["f"] - tether) / np.abs(tether), np.abs(after["f"]))
        _note(worst, "df/f", rel.max())
        assert np.all(np.abs(after["f"] - tether) <= 1e-9 * np.abs(tether)), f"{what}: f is not -k (x - x0), off by {rel.max():.3e} relative"
    else:
        assert _same(after["f"], before["f"]), f"{what}: f changed"
    for key in _ENERGIES:
        _energies_close(f"{what}: {key}", before[key], after[key], want[key], worst)
    for j in range(2):
        _energies_close(f"{what}: parts[{j}]", before["parts"][j], after["parts"][j], want["parts"][j], worst)
    for key in _EXACT:
        assert _same(after[key], want[key]), f"{what}: {key} is {after[key]}, expected {want[key]}"


def _check_front(what, before, after, part):
    """What must hold behind `tethers` and `pre` whatever the restatement says."""
    assert np.array_equal(after["step"], before["step"]), f"{what}: the step word moved"
    for key in ("energy", "acc", "done", "last", "log_pe", "log_ke"):
        assert _same(after[key], before[key]), f"{what}: {key} changed"
    assert _same(after["parts"][1 - part], before["parts"][1 - part]) and np.all(np.isfinite(after["parts"][part]))


def _check_back(what, before, after):
    """What must hold behind `post` and `mid` whatever the restatement says."""
    R, cap = len(before["step"]), before["capacity"]
    assert np.array_equal(after["step"], before["step"] + 1), f"{what}: step"
    assert np.all(_bits(after["energy"]) == 0) and np.all(_bits(after["acc"][:, 0]) == 0) and np.all(after["done"] == 0), what
    assert _same(after["acc"][:, 1], before["acc"][:, 1]) and np.all(after["acc"][:, 1] == mr.ACC1), f"{what}: acc[r][1]"
    assert np.all(np.isfinite(after["last"])), f"{what}: last"
    for key in ("log_pe", "log_ke"):
        changed = np.flatnonzero(_bits(after[key]) != _bits(before[key]))
        slots = [r * cap + int(s) for r, s in enumerate(before["step"]) if s < cap]
        assert list(changed) == slots, f"{what}: {key} was written at {list(changed)}, expected {slots}"
        assert _same(after[key][R * cap:], before[key][R * cap:]), f"{what}: the tail of {key}"


SEQUENCES = [(kind, n, R) for kind in (LANGEVIN, VERLET) for n, R in CASES] + [(VERLET, 65537, 2)]  # (257 blocks per replica)


def _evaluate(dev, y0, energy=True):
    """The stand-in for the evaluation, made on the host from the positions read back: f += F, energy = E uploaded."""
    s = dev.read()
    F, E = mr.standin(s["x"], y0)
    dev.upload("f", s["f"] + F)
    if energy:
        dev.upload("energy", E)


@pytest.mark.parametrize("kind,n,R", SEQUENCES, ids=[f"{'langevin' if k == LANGEVIN else 'verlet'}-n{n}-R{R}" for k, n, R in SEQUENCES])
def test_every_launch_of_three_steps_is_its_restatement(gpu, kind, n, R):
    """tethers, (forces of the stand-in), pre, evaluation, mid, evaluation, mid, evaluation, post: three steps with the partial
    buffers alternating as `_Replicas.steps` alternates them, every launch compared on its own.  Logs of capacity 8 (plus a
    tail): replica 0 starts at step 5 and fills the last three slots, replica 1 at 7 (one slot written, two refused), replica 2
    at 2^32 + 3 (all refused, the high counter word in use), the others at 0."""
    base = mr.synthetic_state(n, R)
    y0 = mr.standin_anchor(base)
    dev = Device(gpu, base)
    worst = {}

    def one(what, name, args, want_of, moved):
        before = dev.read()
        assert dev.launch(name, *args) == 0
        after = dev.read()
        compare(f"{what} ({name})", before, after, want_of(before), moved, worst)
        return before, after

    before, after = one("start", "tethers", (Part(0),), lambda s: mr.tethers(s, 0), "f")
    _check_front("tethers", before, after, 0)
    _evaluate(dev, y0, energy=False)  # (as _Replicas.forces leaves it: tethers + the evaluation's forces, the energy word zero)
    before, after = one("step 0", "pre", (kind, Part(0)), lambda s: mr.pre(s, kind, 0), "xvf")
    _check_front("pre", before, after, 0)
    for j in range(3):
        _evaluate(dev, y0)
        old, new = j % 2, (j + 1) % 2
        if j < 2:
            before, after = one(f"step {j}", "mid", (kind, Part(old), Part(new)), lambda s: mr.mid(s, kind, old, new), "xvf")
            assert _same(after["parts"][old], before["parts"][old])
        else:
            before, after = one(f"step {j}", "post", (Part(old),), lambda s: mr.post(s, old), "v")
            assert _same(after["parts"][0], before["parts"][0]) and _same(after["parts"][1], before["parts"][1])
        _check_back(f"step {j}", before, after)
    final = dev.read()
    cap = base["capacity"]
    want_slots = [r * cap + s for r in range(R) for s in range(int(base["step"][r]), int(base["step"][r]) + 3) if s < cap]
    assert list(np.flatnonzero(np.isfinite(final["log_pe"]))) == want_slots == list(np.flatnonzero(np.isfinite(final["log_ke"])))
    assert list(final["step"]) == [int(s) + 3 for s in base["step"]]
    print(f"n {n} R {R} kind {kind}: " + "  ".join(f"{key} {val:.2e}" for key, val in sorted(worst.items())))


@pytest.mark.parametrize("kind", [LANGEVIN, VERLET], ids=["langevin", "verlet"])
@pytest.mark.parametrize("n,R", [(257, 3), (64, 1)])
def test_mid_is_post_then_pre_bit_for_bit(gpu, kind, n, R):
    """Two device copies of one state in front of a back half: `mid` on one, `post` then `pre` on the other.  The source runs
    the same operations in the same order, so x, v, f, the new partials, the potential energy, the step words and everything
    handed back are expected bit for bit.  The kinetic energy is the exception where a replica has more than one workgroup: its
    per-block sums meet in an FP64 atomic in the order of arrival."""
    base = mr.synthetic_state(n, R)
    y0 = mr.standin_anchor(base)
    a = Device(gpu, base)
    assert a.launch("tethers", Part(0)) == 0
    _evaluate(a, y0, energy=False)
    assert a.launch("pre", kind, Part(0)) == 0
    _evaluate(a, y0)
    start = a.read()
    b = Device(gpu, start)
    assert a.launch("mid", kind, Part(0), Part(1)) == 0
    assert b.launch("post", Part(0)) == 0
    assert b.launch("pre", kind, Part(1)) == 0
    one, two = a.read(), b.read()
    assert not _same(one["x"], start["x"]) and np.array_equal(one["step"], start["step"] + 1)
    for key in ("x", "v", "f", "step", "energy", "acc", "done", "log_pe"):
        assert _same(one[key], two[key]), f"{key} differs between mid and post + pre"
    assert _same(one["parts"][0], two["parts"][0]) and _same(one["parts"][1], two["parts"][1])
    assert _same(one["last"][:, 0], two["last"][:, 0])
    if mr.blocks(n) == 1:
        assert _same(one["log_ke"], two["log_ke"]) and _same(one["last"][:, 1], two["last"][:, 1])
    else:
        assert np.array_equal(np.isfinite(one["log_ke"]), np.isfinite(two["log_ke"]))
        for e, eo in zip(one["log_ke"][np.isfinite(one["log_ke"])], two["log_ke"][np.isfinite(two["log_ke"])]):
            energy_close(e, eo)
        for e, eo in zip(one["last"][:, 1], two["last"][:, 1]):
            energy_close(e, eo)


def _core_state(gpu, core):
    gpu.torch.cuda.synchronize()
    cpu = lambda t: t.cpu().numpy()  # noqa: E731
    return dict(x=cpu(core.x), v=cpu(core.v), f=cpu(core.frc), x0=cpu(core.x0), hdt_m=cpu(core.hdt_m1), mass=cpu(core.mass1), kT=cpu(core.kT),
                seeds=cpu(core.seed_words).view(np.uint64), c1=core.c1, dt=core.dt, k=core.k, energy=cpu(core.e_agbnp), acc=cpu(core.acc),
                done=cpu(core.done).view(np.uint32), step=cpu(core.counter), last=cpu(core.last), log_pe=cpu(core.log_pe).reshape(-1),
                log_ke=cpu(core.log_ke).reshape(-1), capacity=core.log_capacity, parts=[cpu(p) for p in core.parts])


@pytest.mark.parametrize("kind", [LANGEVIN, VERLET], ids=["langevin", "verlet"])
def test_the_drivers_sequencing_is_the_chained_restatement(gpu, kind):
    """md._Replicas itself on a namespace for a system (n = 257, R = 3), its `evaluate` the harmonic stand-in in torch operations
    on the stream it is given: forces(), then steps(kind, c) for c = 1, 2, 3 back to back against the restatement chained from
    the start (pre, (evaluation, mid)..., evaluation, post with parts[j % 2]), at the bounds of this file.  The log holds 4 steps
    of the 6.  Forces behind an evaluation are tethers + stand-in: 1e-9 of the larger of the two terms, elementwise."""
    torch, md = gpu.torch, gpu.md
    n, R, cap = 257, 3, 4
    base = mr.synthetic_state(n, R)
    y0 = mr.standin_anchor(base)
    system = types.SimpleNamespace(n=n, pos=base["x0"], ishydrogen=(base["mass"] < 2.0).astype(np.int32))
    core = md._Replicas(torch, system, [280.0 + 20.0 * r for r in range(R)], [mr.seed_word(r) for r in range(R)], base["k"], base["dt"], 10.0,
                        "cuda:0", cap)
    core.x.copy_(_up(gpu, base["x"]))
    y0_t = _up(gpu, y0)
    side = torch.cuda.Stream(device=gpu.dev)

    def evaluate(st):
        assert st == torch.cuda.current_stream().cuda_stream == side.cuda_stream
        d = core.x - y0_t
        core.frc.sub_(d, alpha=mr.K2)
        core.e_agbnp.add_((d * d).sum(dim=(1, 2)), alpha=0.5 * mr.K2)

    def check(what, before, want, moved):
        after = _core_state(gpu, core)
        worst = {}
        for key, tol in (("x", 1e-11), ("v", 1e-9)):
            d = np.abs(after[key] - want[key]).max()
            _note(worst, "d" + key, d)
            assert (d < tol) if key in moved else _same(after[key], before[key]), f"{what}: {key} differs by {d:.3e}"
        tether, F = -base["k"] * (after["x"] - after["x0"][None]), mr.standin(after["x"], y0)[0]
        assert np.all(np.abs(after["f"] - (tether + F)) <= 1e-9 * np.maximum(np.abs(tether), np.abs(F))), f"{what}: f"
        for key in _ENERGIES:
            _energies_close(f"{what}: {key}", before[key], after[key], want[key], worst)
        for j in range(2):
            _energies_close(f"{what}: parts[{j}]", before["parts"][j], after["parts"][j], want["parts"][j], worst)
        for key in _EXACT:
            assert _same(after[key], want[key]), f"{what}: {key} is {after[key]}, expected {want[key]}"
        print(f"{what}: " + "  ".join(f"{key} {val:.2e}" for key, val in sorted(worst.items())))
        return after

    torch.cuda.synchronize()
    before = _core_state(gpu, core)
    want = mr.copy_state(before)  # the restatement's chain starts at the driver's start (its velocities are torch's draw)
    with torch.cuda.stream(side):
        core.forces(torch, side.cuda_stream, evaluate)
    want = mr.evaluated(mr.tethers(want, 0), y0)
    want["last"][:, 0] = (want["parts"][0].astype(np.longdouble).sum(axis=1) + want["energy"]).astype(np.float64)
    want["energy"][:] = 0.0
    before = check("forces", before, want, "")
    done = 0
    for c in (1, 2, 3):
        with torch.cuda.stream(side):
            core.steps(kind, c, side.cuda_stream, evaluate)
        want = mr.pre(want, kind, 0)
        for j in range(c):
            want = mr.evaluated(want, y0)
            want = mr.mid(want, kind, j % 2, (j + 1) % 2) if j + 1 < c else mr.post(want, j % 2)
        done += c
        before = check(f"steps({c})", before, want, "xv")
        assert list(before["step"]) == [done] * R
    assert np.all(before["log_pe"] != 0.0) and np.all(before["log_ke"] > 0.0)  # 4 of the 6 steps: every slot of the log


def test_bad_arguments_are_refused_and_touch_nothing(gpu):
    """A null struct, n = 0, replicas = 0 and replicas = 17: each of the four group entry points and agbnp_md_exchange returns
    non-zero, and after a synchronisation no word of the state has changed."""
    md, lib, torch = gpu.md, gpu.lib, gpu.torch
    dev = Device(gpu, mr.evaluated(mr.synthetic_state(65, 2), mr.standin_anchor(mr.synthetic_state(65, 2))))
    ex = Exchange(gpu, mr.exchange_state(65, 2))
    ex.upload_energies(np.array([-1000.0, -990.0]))
    before, ex_before = dev.read(), ex.read()

    for fields in (None, dict(n=0), dict(replicas=0), dict(replicas=17)):
        g = None if fields is None else altered(dev.g, **fields)
        assert dev.launch("tethers", Part(0), g=g) != 0, fields
        assert dev.launch("pre", LANGEVIN, Part(0), g=g) != 0, fields
        assert dev.launch("mid", VERLET, Part(0), Part(1), g=g) != 0, fields
        assert dev.launch("post", Part(0), g=g) != 0, fields
        e = None if fields is None else altered(ex.e, **fields)
        assert lib.agbnp_md_exchange(e, torch.cuda.current_stream().cuda_stream) != 0, fields
    torch.cuda.synchronize()
    after, ex_after = dev.read(), ex.read()
    for key in before:
        if key == "parts":
            assert _same(after[key][0], before[key][0]) and _same(after[key][1], before[key][1])
        elif isinstance(before[key], np.ndarray):
            assert _same(after[key], before[key]), key
    for key in ex_before:
        if isinstance(ex_before[key], np.ndarray):
            assert ex_after[key].tobytes() == ex_before[key].tobytes(), key
    # and the unaltered structs are accepted
    assert dev.launch("tethers", Part(1)) == 0 and ex.attempt() == 0


# ---- the exchange kernels alone ------------------------------------------------------------------------------------------------------

class Exchange:
    """The exchange's words as device tensors, the records in a `record_buffer`."""

    def __init__(self, gpu, state):
        self.gpu, self.base = gpu, state
        self.R, self.n = state["v"].shape[:2]
        self.t = t = {key: _up(gpu, state[key]) for key in ("v", "kT", "rung_of_replica", "replica_at_rung", "last", "step", "attempts", "scale")}
        t["records"], log = record_buffer(gpu, state, gpu.md.EXCHANGE_RECORD)
        self.e = gpu.md._args(gpu.md._ExchangeArgs, n=self.n, replicas=self.R, log=log, log_capacity=state["log_capacity"],
                              seed=mr.EXCHANGE_SEED, **{key: val for key, val in t.items() if key != "records"})
        gpu.torch.cuda.synchronize()

    def upload_energies(self, u):
        last = self.t["last"].cpu().numpy().copy()
        last[:, 0] = u
        self.t["last"].copy_(self.gpu.torch.from_numpy(last))

    def read(self):
        self.gpu.torch.cuda.synchronize()
        out = {key: val for key, val in self.base.items() if not isinstance(val, np.ndarray)}
        out.update({key: val.cpu().numpy().copy() for key, val in self.t.items()})
        return split_records(out, self.gpu.md.EXCHANGE_RECORD)

    def attempt(self):
        torch = self.gpu.torch
        torch.cuda.synchronize()
        rc = self.gpu.lib.agbnp_md_exchange(C.byref(self.e), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc


def _exchange_run(gpu, n, R, **kw):
    """64 attempts from a = 2^32 - 3, fresh energies in front of each; after every attempt, against the restatement: kT, rungs,
    attempts and scale bit for bit, the whole record buffer byte for byte (every field of every record at its place, the deviate,
    the energies and the verdict among them, 0xFF wherever nothing was to be written), velocities old value times scale to 1e-15
    relative elementwise and untouched where scale is 1; `last` and `step` are read only."""
    ex = Exchange(gpu, mr.exchange_state(n, R, **kw))
    energies = mr.exchange_energies(R)
    took = tried = 0
    for i, u in enumerate(energies):
        ex.upload_energies(u)
        before = ex.read()
        del before["guards"]
        assert ex.attempt() == 0
        after, want = ex.read(), mr.exchange(before, mr.EXCHANGE_SEED)
        what = f"attempt {i}"
        for key in ("kT", "rung_of_replica", "replica_at_rung", "attempts", "scale", "last", "step"):
            assert after[key].tobytes() == want[key].tobytes(), f"{what}: {key} is {after[key]}, expected {want[key]}"
        assert int(after["attempts"][0]) == mr.FIRST_ATTEMPT + i + 1
        if after["records"].tobytes() != want["records"].tobytes():
            bad = [j for j in range(len(want["records"])) if after["records"][j].tobytes() != want["records"][j].tobytes()]
            raise AssertionError(f"{what}: records {bad[:4]} are {after['records'][bad[:4]]}, expected {want['records'][bad[:4]]}")
        assert set(after["guards"].tobytes()) == {0xFF}, f"{what}: a record was written outside the buffer"
        for r in range(R):
            if want["scale"][r] == 1.0:
                assert _same(after["v"][r], before["v"][r]), f"{what}: v[{r}] changed"
            else:
                scaled = before["v"][r] * want["scale"][r]
                assert np.all(np.abs(after["v"][r] - scaled) <= 1e-15 * np.abs(scaled)), f"{what}: v[{r}]"
                assert not _same(after["v"][r], before["v"][r])
        tried += len(range((mr.FIRST_ATTEMPT + i) & 1, R - 1, 2))
        took += int((want["scale"] != 1.0).sum()) // 2
    return ex.read(), tried, took


@pytest.mark.parametrize("n", [1, 257])
@pytest.mark.parametrize("R", [2, 3, 5, 16])
def test_every_exchange_attempt_is_its_restatement(gpu, n, R):
    """tests/test_md_restatement.py shows for these inputs that no verdict hangs on the last bits and that both verdicts occur,
    so every record is judged.  Odd R (the last rung sits out even attempts), R = 16, the attempt number crossing 2^32."""
    final, tried, took = _exchange_run(gpu, n, R)
    assert tried == len(final["records"]) == mr.exchange_places(mr.FIRST_ATTEMPT + 64, R) - mr.exchange_places(mr.FIRST_ATTEMPT, R)
    assert int(final["records"]["accepted"].sum()) == took and 0 < took < tried
    assert set(final["records"]["attempt"]) == {a for a in range(mr.FIRST_ATTEMPT, mr.FIRST_ATTEMPT + 64) if R > 2 or a % 2 == 0}
    assert np.array_equal(final["records"]["step"], 1000 + 7 * final["records"]["replica_lo"])
    print(f"n {n} R {R}: {took} of {tried} exchanges accepted")


def test_a_truncated_exchange_log_keeps_the_decisions(gpu):
    """log_capacity = 40 records over a buffer of 160 full of 0xFF, R = 5: places from 40 on stay 0xFF while kT and the rungs
    follow the restatement through all 64 attempts (_exchange_run compares them and the whole buffer after every attempt)."""
    final, tried, took = _exchange_run(gpu, 257, 5, log_capacity=40, buffer=160)
    assert tried == 128 and len(final["records"]) == 160
    assert set(final["records"][40:].tobytes()) == {0xFF}
    assert np.all(final["records"]["attempt"][:40] >= mr.FIRST_ATTEMPT) and int(final["attempts"][0]) == mr.FIRST_ATTEMPT + 64
    assert sorted(final["rung_of_replica"]) == list(range(5)) and 0 < took < tried


@pytest.mark.parametrize("n", [1, 257])
def test_one_replica_has_nobody_to_exchange_with(gpu, n):
    """R = 1: 64 attempts change nothing but the attempt counter (scale starts at the 1 every attempt resets it to)."""
    state = mr.exchange_state(n, 1)
    state["scale"][:] = 1.0
    ex = Exchange(gpu, state)
    ex.upload_energies(np.array([-1000.0]))
    before = ex.read()
    for _ in range(64):
        assert ex.attempt() == 0
    after = ex.read()
    assert int(after["attempts"][0]) == mr.FIRST_ATTEMPT + 64
    for key in before:
        if isinstance(before[key], np.ndarray) and key != "attempts":
            assert after[key].tobytes() == before[key].tobytes(), key
