"""GPU box: the lambda-exchange launch of csrc/md_kernels.hip alone (agbnp_md_lambda_exchange: one workgroup decides and swaps),
one attempt at a time, against the CPU restatement of tests/lambda_exchange_restatement.py (long double; checked against itself
by tests/test_lambda_exchange_api.py).  No engine: the state is synthetic.  In front of every attempt the whole state is uploaded,
after it the whole state is read back; the "before" goes to the restatement and the "after" is compared with its prediction:

  bit for bit       every integer word (both maps, the attempt counter, step), every lambda word, kT, u (all R words zero
                    behind an attempt), every copied double and the deviate of a record, every tail behind an array, the log
                    places of other attempts, those beyond the capacity and the guard records around the buffer
  the verdict       wherever |log(uniform) - Delta| > 1e-9 max(1, |Delta|): tests/test_lambda_exchange_api.py shows on the CPU
                    that this is EVERY record of these inputs, and the tests here assert that none was left out."""
import ctypes as C

import numpy as np
import pytest

from tests import lambda_exchange_restatement as lr
from tests import md_restatement as mr
from tests.md_kernel_harness import _OWN, _same, _up, altered, gpu, record_buffer, split_records  # noqa: F401

pytestmark = pytest.mark.gpu

_ARRAYS = ("lambda", "u", "kT", "step", "rung_of_replica", "replica_at_rung", "attempts")
_RECORD_FIELDS = ("attempt", "step", "rung", "replica_lo", "replica_hi", "u_lo", "u_hi", "lambda_lo", "lambda_hi", "kT_lo", "kT_hi", "uniform")


class Device:
    """A restatement state as device tensors, the records in a `record_buffer`, and the argument struct over them."""

    def __init__(self, gpu, state):
        self.gpu, self.base = gpu, state
        self.t = t = {key: _up(gpu, state[key]) for key in _ARRAYS}
        words = dict(t)
        t["records"], log = record_buffer(gpu, state, gpu.md.LAMBDA_RECORD)
        self.e = gpu.md._args(gpu.md._LambdaArgs, replicas=state["replicas"], log=log, log_capacity=state["log_capacity"],
                              seed=lr.EXCHANGE_SEED, **words)
        gpu.torch.cuda.synchronize()

    def upload(self, state):
        """Every array of `state` but the records, which only the kernel writes."""
        for key in _ARRAYS:
            self.t[key].copy_(self.gpu.torch.from_numpy(np.ascontiguousarray(state[key])))

    def read(self):
        self.gpu.torch.cuda.synchronize()
        out = {key: val for key, val in self.base.items() if not isinstance(val, np.ndarray)}
        out.update({key: val.cpu().numpy().copy() for key, val in self.t.items()})
        return split_records(out, self.gpu.md.LAMBDA_RECORD)

    def attempt(self, e=_OWN):
        torch = self.gpu.torch
        torch.cuda.synchronize()
        rc = self.gpu.lib.agbnp_md_lambda_exchange(C.byref(self.e) if e is _OWN else e, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc


def compare(what, before, after, want, tally):
    """The state after one attempt against the restatement's prediction."""
    R = int(before["replicas"])
    for key in _ARRAYS:
        assert _same(after[key], want[key]), f"{what}: {key} is {after[key]}, expected {want[key]}"
    for key in ("kT", "step"):
        assert _same(after[key], before[key]), f"{what}: {key} changed"
    for key in _ARRAYS:  # (the restatement's prediction keeps the tails: said again against the input)
        tail = 1 if key == "attempts" else R
        assert _same(after[key][tail:], before[key][tail:]), f"{what}: the tail of {key}"
    assert set(after["guards"].tobytes()) == {0xFF}, f"{what}: a record was written outside the buffer"
    a = int(before["attempts"][0])
    first = mr.exchange_places(a, R) - before["record_base"]
    mine = [first + t for t in range(len(lr.pairs(a, R))) if first + t + before["record_base"] < before["log_capacity"]]
    for place in range(len(want["records"])):
        got, exp = after["records"][place], want["records"][place]
        if place not in mine:
            assert got.tobytes() == exp.tobytes() == before["records"][place].tobytes(), f"{what}: record place {place} changed"
            continue
        for key in _RECORD_FIELDS:
            assert got[key].tobytes() == exp[key].tobytes(), f"{what}: record {place}: {key} is {got[key]}, expected {exp[key]}"
        tally["records"] += 1
        if exp["accepted"] < 0:
            assert got["accepted"] == -1, f"{what}: record {place}: a void pair was judged"
            tally["void"] += 1
            continue
        margin, delta = lr.margin(got)
        if margin > lr.BAND:
            assert got["accepted"] == exp["accepted"], f"{what}: record {place}: verdict {got['accepted']} for Delta {delta}, uniform {got['uniform']}"
        else:
            tally["unjudged"] += 1
            assert got["accepted"] in (0, 1)
        tally["accepted"] += int(got["accepted"] == 1)


def _run(gpu, R, **kw):
    """lr.ATTEMPTS attempts from a = 2^32 - 3 (both parities, the carry into the counter's high word), fresh u words in front
    of each (lr.energies), chained through the device's own maps, lambdas, counter and records."""
    state = lr.lambda_state(R, **kw)
    dev = Device(gpu, state)
    tally = dict(records=0, unjudged=0, accepted=0, void=0)
    for i in range(lr.ATTEMPTS):
        before = lr.energies(state, i)
        dev.upload(before)
        before = dev.read()
        del before["guards"]
        assert int(before["attempts"][0]) == lr.FIRST_ATTEMPT + i
        assert dev.attempt() == 0
        after = dev.read()
        compare(f"R {R} attempt {i}", before, after, lr.exchange(before, lr.EXCHANGE_SEED), tally)
        state = {key: val for key, val in after.items() if key != "guards"}
    assert tally["unjudged"] == 0  # no case may be left out
    return state, tally


@pytest.mark.parametrize("R", lr.SIZES)
def test_every_attempt_is_its_restatement(gpu, R):
    """R = 1 (no pair: only the counter moves), 2 (odd attempts have none), 3 (replica on rung 0 or 2 sits out), 8 and 16 (the
    first 8 or 7 threads have a pair)."""
    final, tally = _run(gpu, R)
    total = mr.exchange_places(lr.FIRST_ATTEMPT + lr.ATTEMPTS, R) - mr.exchange_places(lr.FIRST_ATTEMPT, R)
    assert tally["records"] == total and int(final["attempts"][0]) == lr.FIRST_ATTEMPT + lr.ATTEMPTS and tally["void"] == 0
    if R == 1:
        assert set(final["records"].tobytes()) == {0xFF}
    else:
        assert 0 < tally["accepted"] < total
    at = final["replica_at_rung"][:R]
    assert sorted(at) == list(range(R)) and np.array_equal(final["rung_of_replica"][:R][at], np.arange(R))
    assert final["lambda"][:R][at].tobytes() == lr.ladder(R).tobytes()  # every rung keeps its lambda
    print(f"R {R}: {tally['accepted']} of {tally['records']} exchanges accepted, {tally['unjudged']} verdicts not judged")


def test_certain_and_void_pairs(gpu):
    """R = 16 in front of an even attempt whose pairs (0,1) .. (10,11) are: Delta = +50 (accepted whatever the deviate is), Delta =
    -50 (rejected), and a u word that is 0.0, -0.0, NaN, -inf (void: accepted = -1, nothing swapped, both u words handed back as
    zeros all the same)."""
    before = lr.crafted_state()
    dev = Device(gpu, before)
    before = dev.read()
    del before["guards"]
    assert dev.attempt() == 0
    after = dev.read()
    tally = dict(records=0, unjudged=0, accepted=0, void=0)
    compare("crafted", before, after, lr.exchange(before, lr.EXCHANGE_SEED), tally)
    assert tally == dict(records=8, unjudged=0, accepted=tally["accepted"], void=4)
    assert list(after["records"]["accepted"][:len(lr.CRAFTED)]) == [1, 0, -1, -1, -1, -1]
    assert list(after["replica_at_rung"][:12]) == [1, 0] + list(range(2, 12))
    assert after["u"][:16].tobytes() == np.zeros(16).tobytes()
    assert after["lambda"][4:12].tobytes() == before["lambda"][4:12].tobytes()


def test_a_log_that_ends_inside_an_attempt(gpu):
    """log_capacity = 12 records over a buffer of all 120 full of 0xFF, R = 16: the first attempt (odd: 7 pairs) fits, the second
    (8 pairs) is cut after its fifth record, every later place stays 0xFF, and the maps and lambdas go on as the restatement's."""
    final, tally = _run(gpu, 16, log_capacity=12)
    assert tally["records"] == 12 and len(final["records"]) == 120
    assert set(final["records"][12:].tobytes()) == {0xFF} and final["records"]["rung"][11] == 8
    assert int(final["attempts"][0]) == lr.FIRST_ATTEMPT + lr.ATTEMPTS and not np.array_equal(final["replica_at_rung"][:16], np.arange(16))


def test_bad_arguments_are_refused_and_touch_nothing(gpu):
    """A null struct, replicas = 0 and 17, a null array: the entry point returns non-zero and no word of the state changes."""
    dev = Device(gpu, lr.energies(lr.lambda_state(3, first_attempt=lr.FIRST_ATTEMPT + 1), 0))
    before = dev.read()
    for fields in (None, dict(replicas=0), dict(replicas=17), dict(replicas=-1), dict(u=None), dict(attempts=None)):
        assert dev.attempt(e=None if fields is None else altered(dev.e, **fields)) != 0, fields
    after = dev.read()
    for key in before:
        if isinstance(before[key], np.ndarray):
            assert after[key].tobytes() == before[key].tobytes(), key
    assert dev.attempt() == 0 and int(dev.read()["attempts"][0]) == lr.FIRST_ATTEMPT + 2  # the unaltered struct is accepted
