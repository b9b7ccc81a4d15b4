"""GPU box: the two Hamiltonian-exchange kernels of csrc/md_kernels.hip alone (agbnp_md_hamiltonian_exchange: decide, then
exchange the conformations), one attempt at a time, against the CPU restatement of tests/hremd_restatement.py (long double; checked
against itself and against md_restatement.exchange by tests/test_hremd_api.py).  No engine: the state is synthetic.  In front of
every attempt the whole state is uploaded, after it the whole state is read back; the "before" goes to the restatement and the
"after" is compared with its prediction word by word:

  x                 bit for bit (a pure swap)
  v                 1e-15 relative elementwise where a conformation arrived, bit for bit elsewhere
  record energies, last[:, 1], scale   tests.gpu_helpers.energy_close (words that are not finite: bit for bit)
  the verdict       where |log u - Delta| >= 1e-12 max(1, |Delta|) (tests/test_hremd_api.py shows that this is everywhere)
  everything else   bit for bit: kT, step, f, last[:, 0], both partial buffers, both maps, the partner words, the attempt counter,
                    cross (zeros where a pair read it), the deviate and the integers of every record, and every sentinel: x and v of
                    the slots that sit an attempt out, the tails of cross / scale / partner, the log places of other attempts, those
                    beyond the capacity and the guard records around the buffer."""
import ctypes as C

import numpy as np
import pytest

from tests import hremd_restatement as hr
from tests import md_restatement as mr
from tests.gpu_helpers import energy_close
from tests.md_kernel_harness import _OWN, _bits, _same, _up, altered, gpu, record_buffer, split_records  # noqa: F401
from tests.test_hremd_api import CASES, CRAFTED, crafted_state

pytestmark = pytest.mark.gpu

_ARRAYS = ("x", "v", "f", "kT", "last", "step", "cross", "scale", "partner", "walker_at_rung", "rung_of_walker", "attempts")
_EXACT = ("x", "f", "kT", "step", "cross", "partner", "walker_at_rung", "rung_of_walker", "attempts")
_RECORD_EXACT = ("attempt", "step", "rung", "walker_lo", "walker_hi", "u")
_RECORD_ENERGIES = ("P_lo", "P_hi", "T_lo", "T_hi", "C_lo", "C_hi", "kT_lo", "kT_hi")


class Device:
    """A restatement state as device tensors, the records in a `record_buffer`, and one argument struct per partial buffer."""

    def __init__(self, gpu, state):
        self.gpu, self.base = gpu, state
        self.R, self.n = state["x"].shape[:2]
        self.t = t = {key: _up(gpu, state[key]) for key in _ARRAYS}
        self.parts = [_up(gpu, p) for p in state["parts"]]
        words = {key: val for key, val in t.items() if key != "f"}  # (f is state the kernels must leave alone, not an argument)
        t["records"], log = record_buffer(gpu, state, gpu.md.HAMILTONIAN_RECORD)
        self.h = [gpu.md._args(gpu.md._HamiltonianArgs, n=self.n, replicas=self.R, tether_part=part, log=log,
                               log_capacity=state["log_capacity"], seed=hr.EXCHANGE_SEED, **words) for part in self.parts]
        gpu.torch.cuda.synchronize()

    def upload(self, state):
        """Every array of `state` but the records, which only the kernel writes."""
        torch = self.gpu.torch
        for key in _ARRAYS:
            self.t[key].copy_(torch.from_numpy(np.ascontiguousarray(state[key])))
        for j in range(2):
            self.parts[j].copy_(torch.from_numpy(np.ascontiguousarray(state["parts"][j])))

    def read(self):
        self.gpu.torch.cuda.synchronize()
        out = {key: val for key, val in self.base.items() if not isinstance(val, (np.ndarray, list))}
        out.update({key: val.cpu().numpy().copy() for key, val in self.t.items()})
        out["parts"] = [p.cpu().numpy().copy() for p in self.parts]
        return split_records(out, self.gpu.md.HAMILTONIAN_RECORD)

    def attempt(self, part, h=_OWN):
        torch = self.gpu.torch
        torch.cuda.synchronize()
        rc = self.gpu.lib.agbnp_md_hamiltonian_exchange(C.byref(self.h[part]) if h is _OWN else h, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc


def _close(what, got, want):
    if np.isfinite(got) and np.isfinite(want):
        energy_close(got, want)
    else:
        assert _bits(np.float64(got)) == _bits(np.float64(want)), f"{what}: {got} for {want}"


def compare(what, before, after, want, tally):
    """The state after one attempt against the restatement's prediction."""
    R = len(before["kT"])
    for key in _EXACT:
        assert _same(after[key], want[key]), f"{what}: {key} is {after[key]}, expected {want[key]}"
    assert _same(after["last"][:, 0], before["last"][:, 0]), f"{what}: last[:, 0] changed"
    for j in range(2):
        assert _same(after["parts"][j], before["parts"][j]), f"{what}: parts[{j}] changed"
    assert set(after["guards"].tobytes()) == {0xFF}, f"{what}: a record was written outside the buffer"
    assert _same(after["scale"][R:], before["scale"][R:]), f"{what}: the tail of scale"
    for r in range(R):
        _close(f"{what}: scale[{r}]", after["scale"][r], want["scale"][r])
        if _bits(want["last"][r, 1]) == _bits(before["last"][r, 1]):
            assert _bits(after["last"][r, 1]) == _bits(before["last"][r, 1]), f"{what}: last[{r}][1] changed"
        else:
            _close(f"{what}: last[{r}][1]", after["last"][r, 1], want["last"][r, 1])
        if want["partner"][r] < 0:
            assert after["scale"][r] == 1.0 and _same(after["v"][r], before["v"][r]), f"{what}: slot {r} sat out and changed"
        else:
            arrived = before["v"][want["partner"][r]] * want["scale"][r]
            assert np.all(np.abs(after["v"][r] - arrived) <= 1e-15 * np.abs(arrived)), f"{what}: v[{r}]"
            if after["scale"][r] == 1.0:
                assert _same(after["v"][r], before["v"][want["partner"][r]])
    # the records: those of this attempt field by field, every other place of the buffer byte for byte
    a = int(before["attempts"][0])
    first = mr.exchange_places(a, R) - before["record_base"]
    mine = [first + t for t in range(len(hr.pairs(a, R))) if first + t + before["record_base"] < before["log_capacity"]]
    for place in range(len(want["records"])):
        got, exp = after["records"][place], want["records"][place]
        if place not in mine:
            assert got.tobytes() == exp.tobytes() == before["records"][place].tobytes(), f"{what}: record place {place} changed"
            continue
        for key in _RECORD_EXACT:
            assert got[key].tobytes() == exp[key].tobytes(), f"{what}: record {place}: {key} is {got[key]}, expected {exp[key]}"
        for key in _RECORD_ENERGIES:
            _close(f"{what}: record {place}: {key}", got[key], exp[key])
        tally["records"] += 1
        margin, delta = hr.margin(got) if exp["accepted"] >= 0 else (np.inf, None)
        if margin >= 1e-12:
            assert got["accepted"] == exp["accepted"], f"{what}: record {place}: verdict {got['accepted']} for Delta {delta}, u {got['u']}"
        else:
            tally["unjudged"] += 1
            assert got["accepted"] in (0, 1)
        tally["accepted"] += int(got["accepted"] == 1)
    return mine


def _run(gpu, n, R, **kw):
    """hr.ATTEMPTS attempts from a = 2^32 - 3, fresh inputs in front of each (hr.energies; the partial buffer in use alternates,
    the other one holds sentinels), chained through the device's own maps, counter and records."""
    state = hr.hamiltonian_state(n, R, **kw)
    dev = Device(gpu, state)
    tally = dict(records=0, unjudged=0, accepted=0)
    for i in range(hr.ATTEMPTS):
        part = i % 2
        before = hr.energies(state, i, part)
        dev.upload(before)
        before = dev.read()
        del before["guards"]
        assert int(before["attempts"][0]) == hr.FIRST_ATTEMPT + i
        assert dev.attempt(part) == 0
        after = dev.read()
        compare(f"n {n} R {R} attempt {i}", before, after, hr.exchange(before, hr.EXCHANGE_SEED, part), tally)
        state = {key: val for key, val in after.items() if key != "guards"}
    assert tally["unjudged"] < 0.01 * max(tally["records"], 1)
    return state, tally


@pytest.mark.parametrize("n,R", CASES)
def test_every_attempt_is_its_restatement(gpu, n, R):
    """n = 1, one full workgroup, a second workgroup with a single atom; R = 1 (no pair), 2 (odd attempts have none), 3 (slot 0
    or slot 2 sits out), 16 (every thread of the deciding workgroup's first 8 or 7 has a pair); the attempt number crosses 2^32."""
    final, tally = _run(gpu, n, R)
    total = mr.exchange_places(hr.FIRST_ATTEMPT + hr.ATTEMPTS, R) - mr.exchange_places(hr.FIRST_ATTEMPT, R)
    assert tally["records"] == total and int(final["attempts"][0]) == hr.FIRST_ATTEMPT + hr.ATTEMPTS
    if R == 1:
        assert set(final["records"].tobytes()) == {0xFF}
    else:
        assert 0 < tally["accepted"] < total
        assert set(final["records"]["attempt"]) == {a for a in range(hr.FIRST_ATTEMPT, hr.FIRST_ATTEMPT + hr.ATTEMPTS) if R > 2 or a % 2 == 0}
        assert np.array_equal(final["records"]["step"], 1000 + 7 * final["records"]["rung"])
    assert sorted(final["walker_at_rung"]) == list(range(R))
    assert np.array_equal(final["rung_of_walker"][final["walker_at_rung"]], np.arange(R))
    print(f"n {n} R {R}: {tally['accepted']} of {tally['records']} exchanges accepted, {tally['unjudged']} verdicts not judged")


@pytest.mark.parametrize("n", [1, 257])
def test_certain_equal_and_void_pairs(gpu, n):
    """R = 16 in front of an even attempt whose pairs (0,1) .. (8,9) are: Delta = +400 (accepted whatever u is), Delta = -400
    (rejected), equal everything (Delta = 0: accepted, both factors exactly 1.0, x and v exchanged bit for bit), a cross word left
    0.0 and one set to inf (void: accepted = -1, nothing moves, the cross words handed back as zeros all the same)."""
    before = crafted_state(n)
    dev = Device(gpu, before)
    before = dev.read()
    del before["guards"]
    assert dev.attempt(1) == 0
    after = dev.read()
    tally = dict(records=0, unjudged=0, accepted=0)
    compare(f"n {n} crafted", before, after, hr.exchange(before, hr.EXCHANGE_SEED, 1), tally)
    assert tally["records"] == 8 and tally["unjudged"] == 0
    assert list(after["records"]["accepted"][:len(CRAFTED)]) == [1, 0, 1, -1, -1]
    assert list(after["partner"][:10]) == [1, 0, -1, -1, 5, 4, -1, -1, -1, -1]
    assert after["scale"][4] == 1.0 == after["scale"][5] and _same(after["x"][4], before["x"][5]) and _same(after["v"][5], before["v"][4])
    assert _same(after["x"][6:10], before["x"][6:10]) and _same(after["v"][6:10], before["v"][6:10])
    assert np.all(_bits(after["cross"][:16]) == 0) and list(after["walker_at_rung"][:10]) == [1, 0, 2, 3, 5, 4, 6, 7, 8, 9]


def test_a_log_that_ends_inside_an_attempt(gpu):
    """log_capacity = 12 records over a buffer of all 120 full of 0xFF, R = 16: the first attempt (odd: 7 pairs) fits, the second
    (8 pairs) is cut after its fifth record, every later place stays 0xFF, and the maps go on as the restatement's (compared
    after every attempt)."""
    final, tally = _run(gpu, 257, 16, log_capacity=12)
    assert tally["records"] == 12 and len(final["records"]) == 120
    assert set(final["records"][12:].tobytes()) == {0xFF} and final["records"]["rung"][11] == 8
    assert int(final["attempts"][0]) == hr.FIRST_ATTEMPT + hr.ATTEMPTS and not np.array_equal(final["walker_at_rung"], np.arange(16))


def test_bad_arguments_are_refused_and_touch_nothing(gpu):
    """A null struct, n = 0, replicas = 0 and replicas = 17: the entry point returns non-zero and no word of the state changes."""
    dev = Device(gpu, hr.energies(hr.hamiltonian_state(65, 2, first_attempt=hr.FIRST_ATTEMPT + 1), 0, 0))
    before = dev.read()
    for fields in (None, dict(n=0), dict(replicas=0), dict(replicas=17)):
        assert dev.attempt(0, h=None if fields is None else altered(dev.h[0], **fields)) != 0, fields
    after = dev.read()
    for key in before:
        if key == "parts":
            assert _same(after[key][0], before[key][0]) and _same(after[key][1], before[key][1])
        elif isinstance(before[key], np.ndarray):
            assert after[key].tobytes() == before[key].tobytes(), key
    assert dev.attempt(0) == 0 and int(dev.read()["attempts"][0]) == hr.FIRST_ATTEMPT + 2  # the unaltered struct is accepted
