"""GPU box: the two kernels of the FIRE minimiser (agbnp_md_fire_back, agbnp_md_fire_front of csrc/md_kernels.hip) alone, one
launch at a time, against the CPU restatement of tests/fire_restatement.py (checked on the CPU by tests/test_fire_restatement.py,
which also shows that the sequences used here meet every branch with verdicts that do not hang on the last bits).  No engine:
the state is synthetic and the evaluation between two launches is md_restatement's harmonic stand-in, made on the host from the
positions read back, as tests/test_gpu_md_kernels.py does.  Before and after every launch the whole state is read back; the
"before" goes to the restatement and the "after" is compared with its prediction word by word:

  x, w             1e-11 nm, 1e-9 nm/ps where the replica moves; bit for bit where it does not
  f                -k (x_device - x0) to 1e-9 relative elementwise
  energies         the tether partials and the logged energy by tests.gpu_helpers.energy_close; the logged energy also at its
                   summation bound
  sums             the four partials per workgroup, b and fmax at the summation bounds the restatement reports
  state words      dt, alpha, npos, iterations, converged, voids, a, the move's dt and the move word: bit for bit
  everything else  bit for bit: v, step, log_pe, log_ke, last, acc, done, the partial buffer not in use, the energy word and the
                   arrival counter (zeros behind a back half), log slots other than the iteration's or beyond the capacity, the
                   guard words around the logs

The measured maxima are printed per case."""
import ctypes as C

import numpy as np
import pytest

from tests import fire_restatement as fr
from tests import md_restatement as mr
from tests.gpu_helpers import energy_close
from tests.md_kernel_harness import _OWN, CASES, Device, Part, _bits, _note, _same, _up, altered, gpu  # noqa: F401

pytestmark = pytest.mark.gpu

_FIRE_F64 = ("w", "fdt", "alpha", "fmax", "coef", "fpart", "log_e", "log_fmax")
_UNTOUCHED = ("v", "step", "log_pe", "log_ke", "last", "acc", "done", "x0", "hdt_m", "mass", "kT", "seeds")  # by either launch
_WORDS = ("fdt", "alpha", "npos", "iterations", "converged", "voids")  # bit for bit behind a back half


class FireDevice(Device):
    """A restatement state with the minimiser's words as device tensors, and both argument structs over them.  The log pointers
    handed over are those of the first slot behind the front guard."""

    def __init__(self, gpu, state):
        super().__init__(gpu, state)
        t = self.t
        t.update({key: _up(gpu, state[key]) for key in _FIRE_F64 + ("npos", "converged", "voids", "iterations")})
        t["arrived"] = _up(gpu, state["arrived"].view(np.int32))
        guard = 8 * state["fguard"]
        self.q = gpu.md._args(gpu.md._FireArgs, dt=t["fdt"], part=t["fpart"], log_e=t["log_e"].data_ptr() + guard,
                              log_fmax=t["log_fmax"].data_ptr() + guard, capacity=state["fcap"],
                              **{key: t[key] for key in ("w", "alpha", "npos", "iterations", "converged", "voids", "fmax", "coef", "arrived")},
                              **{key: state[key] for key in ("dt_max", "f_inc", "f_dec", "alpha0", "f_alpha", "n_min", "tolerance", "max_move")})
        gpu.torch.cuda.synchronize()

    def read(self):
        out = super().read()
        out["arrived"] = out["arrived"].view(np.uint32)
        return out

    def fire(self, name, part, g=_OWN, q=_OWN):
        """agbnp_md_fire_<name> on the current stream, waited for; returns its code."""
        torch = self.gpu.torch
        torch.cuda.synchronize()
        rc = getattr(self.gpu.lib, "agbnp_md_fire_" + name)(C.byref(self.g) if g is _OWN else g, C.byref(self.q) if q is _OWN else q,
                                                             self.parts[part].data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc


def _unchanged(what, before, after, keys):
    for key in keys:
        if key == "parts":
            assert _same(after[key][0], before[key][0]) and _same(after[key][1], before[key][1]), f"{what}: parts changed"
        else:
            assert _same(after[key], before[key]), f"{what}: {key} changed"


def check_back(what, before, after, want, bounds, worst):
    """The state behind one back half against the restatement's prediction."""
    R, cap, guard = len(before["x"]), before["fcap"], before["fguard"]
    _unchanged(what, before, after, _UNTOUCHED + ("x", "w", "f", "parts"))
    for key in _WORDS + ("energy", "arrived"):
        assert _same(after[key], want[key]), f"{what}: {key} is {after[key]}, expected {want[key]}"
    assert np.all(_bits(after["energy"]) == 0) and np.all(after["arrived"] == 0), what
    for j in (0, 2, 3):
        assert _same(after["coef"][:, j], want["coef"][:, j]), f"{what}: coef[:, {j}] is {after['coef'][:, j]}, expected {want['coef'][:, j]}"
    off = np.abs(after["fpart"] - want["fpart"])
    with np.errstate(invalid="ignore", divide="ignore"):
        _note(worst, "partials/bound", np.nanmax(np.where(bounds["fpart"] > 0, off / bounds["fpart"], 0.0)))
    assert np.all(off <= bounds["fpart"]), f"{what}: a partial is {off.max():.3e} off"
    for r in range(R):
        branch = bounds["branch"][r]
        slot = guard + r * cap + int(before["iterations"][r])
        written = branch in ("positive", "negative", "done")
        if branch in ("positive", "negative"):
            d = abs(after["coef"][r, 1] - want["coef"][r, 1])
            _note(worst, "b/bound", d / bounds["b"][r] if bounds["b"][r] else d)
            assert d <= bounds["b"][r], f"{what}: b[{r}] is {d:.3e} off, allowed {bounds['b'][r]:.3e}"
        else:
            assert _same(after["coef"][r, 1], before["coef"][r, 1]), f"{what}: b[{r}] changed"
        if written:
            d = abs(after["fmax"][r] - want["fmax"][r])
            _note(worst, "fmax/bound", d / bounds["fmax"][r])
            assert d <= bounds["fmax"][r], f"{what}: fmax[{r}] is {d:.3e} off, allowed {bounds['fmax'][r]:.3e}"
        else:
            assert _same(after["fmax"][r], before["fmax"][r]), f"{what}: fmax[{r}] changed"
        for key in ("log_e", "log_fmax"):
            changed = np.flatnonzero(_bits(after[key]) != _bits(before[key]))
            mine = changed[(changed >= guard + r * cap) & (changed < guard + (r + 1) * cap)]
            assert list(mine) == ([slot] if written and before["iterations"][r] < cap else []), f"{what}: {key} of replica {r} written at {mine}"
        if written and before["iterations"][r] < cap:
            e, eo = after["log_e"][slot], want["log_e"][slot]
            _note(worst, "E/bound", abs(e - eo) / bounds["E"][r])
            energy_close(e, eo)
            assert abs(e - eo) <= bounds["E"][r], f"{what}: E[{r}] is {abs(e - eo):.3e} off, allowed {bounds['E'][r]:.3e}"
            assert _same(after["log_fmax"][slot], after["fmax"][r])
    for key in ("log_e", "log_fmax"):
        assert _same(after[key][:guard], before[key][:guard]) and _same(after[key][guard + R * cap:], before[key][guard + R * cap:]), f"{what}: guards of {key}"


def check_front(what, before, after, want, part, worst):
    """The state behind one front half against the restatement's prediction."""
    R = len(before["x"])
    _unchanged(what, before, after, _UNTOUCHED + _WORDS + ("energy", "arrived", "fmax", "coef", "fpart", "log_e", "log_fmax"))
    assert _same(after["parts"][1 - part], before["parts"][1 - part]), f"{what}: the other partial buffer changed"
    for r in range(R):
        if before["coef"][r, 3] != 0.0:
            dx, dw = np.abs(after["x"][r] - want["x"][r]).max(), np.abs(after["w"][r] - want["w"][r]).max()
            _note(worst, "dx", dx), _note(worst, "dw", dw)
            assert dx < 1e-11 and dw < 1e-9, f"{what}: replica {r}: x differs by {dx:.3e}, w by {dw:.3e}"
            step = np.sqrt(((after["x"][r] - before["x"][r]) ** 2).sum(axis=1)).max()
            assert step <= before["max_move"] * (1.0 + 1e-9), f"{what}: an atom of replica {r} moved {step:.3e} nm"
        else:
            assert _same(after["x"][r], before["x"][r]) and _same(after["w"][r], before["w"][r]), f"{what}: replica {r} did not move and changed"
    tether = -before["k"] * (after["x"] - after["x0"][None])
    assert np.all(np.abs(after["f"] - tether) <= 1e-9 * np.abs(tether)), f"{what}: f is not -k (x - x0)"
    for e, eo in zip(after["parts"][part].ravel(), want["parts"][part].ravel()):
        _note(worst, "dT", abs(e - eo))
        energy_close(e, eo)


def _evaluate(dev, y0, void=()):
    """The stand-in evaluation made on the host from the positions read back: f += F, the energy word = E (zero for `void`)."""
    s = dev.read()
    F, E = mr.standin(s["x"], y0)
    E[list(void)] = 0.0
    dev.upload("f", s["f"] + F)
    dev.upload("energy", E)


SEQUENCES = [(n, R, fr.ITERATIONS) for n, R in CASES] + [(65537, 2, 12)]  # (257 blocks per replica)


@pytest.mark.parametrize("n,R,iterations", SEQUENCES, ids=[f"n{n}-R{R}" for n, R, _ in SEQUENCES])
def test_every_launch_of_a_minimisation_is_its_restatement(gpu, n, R, iterations):
    """tethers, evaluation, then (back, front, evaluation) per iteration as `_Replicas.minimise` enqueues them, every launch
    compared on its own.  Replica 0's evaluation of iteration VOID_AT is withheld (its energy word uploaded as 0.0): that
    iteration changes nothing of replica 0 but voids[0], f and the partials.  The last replica of R >= 2 converges within the
    sequence: from then on its x and w keep their bits over every launch.  Logs of 16 slots between guards: replica 1 starts at
    slot 10 (the last six written, then refused), replica 2 at 2^32 + 3 (all refused)."""
    base, y0 = fr.synthetic_state(n, R)
    dev = FireDevice(gpu, base)
    worst, frozen, seen = {}, {}, set()
    assert dev.launch("tethers", Part(0)) == 0
    _evaluate(dev, y0)
    for it in range(iterations):
        what = f"iteration {it}"
        start = dev.read()
        bounds = {}
        want = fr.back(start, 0, bounds)
        assert dev.fire("back", 0) == 0
        judged = dev.read()
        check_back(what + " (back)", start, judged, want, bounds, worst)
        assert dev.fire("front", 0) == 0
        moved = dev.read()
        check_front(what + " (front)", judged, moved, fr.front(judged, 0), 0, worst)
        seen.update(bounds["branch"])
        for r, (x, w) in frozen.items():
            assert _same(moved["x"][r], x) and _same(moved["w"][r], w), f"{what}: converged replica {r} moved"
        for r in range(R):
            if judged["converged"][r] and r not in frozen:
                frozen[r] = (judged["x"][r].copy(), judged["w"][r].copy())
        if it == fr.VOID_AT:
            assert bounds["branch"][0] == "void" and judged["voids"][0] == start["voids"][0] + 1
            for key in ("x", "w", "fdt", "alpha", "npos", "iterations", "converged", "fmax"):
                assert _same(moved[key][0], start[key][0]), f"the void iteration changed {key}[0]"
            assert _same(moved["coef"][0, :3], start["coef"][0, :3]) and moved["coef"][0, 3] == 0.0
            cap, guard = base["fcap"], base["fguard"]
            for key in ("log_e", "log_fmax"):
                assert _same(moved[key][guard:guard + cap], start[key][guard:guard + cap]), f"the void iteration wrote {key} of replica 0"
        _evaluate(dev, y0, void=(0,) if it + 1 == fr.VOID_AT else ())
    final = dev.read()
    assert {"positive", "negative", "void"} <= seen
    assert final["voids"][0] == 1 and not final["voids"][1:].any()
    if R >= 2:
        assert list(frozen) == [R - 1] and "done" in seen and "converged" in seen
        assert final["iterations"][0] == base["iterations"][0] + iterations - 1
    print(f"n {n} R {R}: " + "  ".join(f"{key} {val:.2e}" for key, val in sorted(worst.items())))


def test_what_is_not_a_number_is_void_and_a_converged_replica_counts_its_voids(gpu):
    """(65, 3) behind one iteration: replica 1 gets a NaN force component beside a finite energy word, replica 2 is marked
    converged and gets a zero energy word.  The back half counts a void for both, moves neither, declares replica 1 not
    converged (max |F_i|^2 alone would not see the NaN) and leaves replica 2 converged; replica 0 goes on.  State words as the
    restatement predicts, bit for bit; x and w of the two replicas keep their bits over the front half."""
    base, y0 = fr.synthetic_state(65, 3)
    dev = FireDevice(gpu, base)
    assert dev.launch("tethers", Part(0)) == 0
    _evaluate(dev, y0)
    assert dev.fire("back", 0) == 0 and dev.fire("front", 0) == 0
    _evaluate(dev, y0)
    s = dev.read()
    s["f"][1, 3, 0] = np.nan
    s["converged"][2], s["energy"][2] = 1, 0.0
    dev.upload("f", s["f"]), dev.upload("converged", s["converged"]), dev.upload("energy", s["energy"])
    before = dev.read()
    want = fr.back(before, 0)
    assert dev.fire("back", 0) == 0
    judged = dev.read()
    for key in _WORDS + ("energy", "arrived"):
        assert _same(judged[key], want[key]), f"{key} is {judged[key]}, expected {want[key]}"
    assert list(judged["voids"]) == [0, 1, 1] and list(judged["converged"]) == [0, 0, 1] and list(judged["coef"][:, 3]) == [1.0, 0.0, 0.0]
    assert _same(judged["fmax"][1:], before["fmax"][1:])
    first = base["fguard"] + base["fcap"]  # (the logs of replicas 1 and 2 and the guard behind them)
    assert _same(judged["log_e"][first:], before["log_e"][first:]) and _same(judged["log_fmax"][first:], before["log_fmax"][first:])
    _unchanged("void", before, judged, _UNTOUCHED + ("x", "w", "f", "parts"))
    assert dev.fire("front", 0) == 0
    moved = dev.read()
    assert _same(moved["x"][1:], before["x"][1:]) and _same(moved["w"][1:], before["w"][1:]) and not _same(moved["x"][0], before["x"][0])


def test_bad_arguments_are_refused_and_touch_nothing(gpu):
    """A null group struct, n = 0, replicas = 0, replicas = 17 and a null minimiser struct: both entry points return non-zero,
    and after a synchronisation no word of the state has changed."""
    base, y0 = fr.synthetic_state(65, 2)
    dev = FireDevice(gpu, mr.evaluated(mr.tethers(base, 0), y0))
    before = dev.read()

    for name in ("back", "front"):
        for fields in (None, dict(n=0), dict(replicas=0), dict(replicas=17)):
            assert dev.fire(name, 0, g=None if fields is None else altered(dev.g, **fields)) != 0, (name, fields)
        assert dev.fire(name, 0, q=None) != 0, name
    after = dev.read()
    for key in before:
        if isinstance(before[key], (np.ndarray, list)):
            _unchanged("refused", before, after, (key,))
    # and the unaltered structs are accepted
    assert dev.fire("back", 0) == 0 and dev.fire("front", 0) == 0
    assert not _same(dev.read()["x"], before["x"])
