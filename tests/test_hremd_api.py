"""HamiltonianReplicaMD (openmm_agbnp_plugin_amd/md.py) at the boundaries that need no device: the host
restatements of the exchange rule and its deviate, the constructor's checks, the library's symbol and struct sizes, and the
restatement of the two kernels (tests/hremd_restatement.py) against itself and against md_restatement.exchange."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from openmm_agbnp_plugin_amd import md
from tests import hremd_restatement as hr
from tests import md_restatement as mr
from tests.test_replica_md_api import _Fake, _System, no_library  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_one_hamiltonian_gives_the_temperature_rule():
    """C_lo = P_hi - T_hi and C_hi = P_lo - T_lo: Delta is exchange_delta(kT_lo, kT_hi, P_lo, P_hi) to 1e-9 for energies up to
    5e4 kJ/mol and kT in 1 .. 5 (the difference is rounding of order 5e4 x 2^-52 / kT = 1e-11)."""
    rng = np.random.default_rng(2)
    worst = 0.0
    for _ in range(500):
        ka, kb = rng.uniform(1.0, 5.0, 2)
        pa, pb = rng.uniform(-5e4, 5e4, 2)
        ta, tb = rng.uniform(0.0, 5e3, 2)
        d = md.hamiltonian_delta(ka, kb, pa, pb, ta, tb, pb - tb, pa - ta)
        worst = max(worst, abs(d - md.exchange_delta(ka, kb, pa, pb)))
    print(f"largest difference {worst:.2e}")
    assert worst < 1e-9


def test_delta_does_not_depend_on_how_the_pair_is_named():
    rng = np.random.default_rng(3)
    for _ in range(200):
        ka, kb = rng.uniform(1.0, 5.0, 2)
        pa, pb, ca, cb = rng.uniform(-5e4, 5e4, 4)
        ta, tb = rng.uniform(0.0, 5e3, 2)
        d = md.hamiltonian_delta(ka, kb, pa, pb, ta, tb, ca, cb)
        other = md.hamiltonian_delta(kb, ka, pb, pa, tb, ta, cb, ca)
        assert abs(other - d) <= 1e-12 * max(1.0, abs(d))  # (the three terms are added in another order)
        # equal baths, every rung seeing the other's conformation as its own: nothing to gain, exactly
        assert md.hamiltonian_delta(ka, ka, pa, pb, ta, tb, pa - ta, pb - tb) == 0.0
    # the rung whose own conformation costs it more than the partner's would is always relieved of it: log(u) <= 0 < Delta
    assert md.hamiltonian_delta(2.0, 3.0, 10.0, -10.0, 1.0, 1.0, -5.0, -11.0) > 0.0
    assert math.log(md.uniform53(0xffffffff, 0xffffffff)) == 0.0


def test_the_deviate_is_the_block_with_counter_word_three():
    w = md.philox4x32((3, 7, 1, 3), (0x12345678, 0x9))
    assert md.hamiltonian_uniform(3, (1 << 32) + 7, (0x9 << 32) | 0x12345678) == md.uniform53(w[0], w[1])
    assert md.hamiltonian_uniform(3, (1 << 32) + 7, (0x9 << 32) | 0x12345678) != md.exchange_uniform(3, (1 << 32) + 7, (0x9 << 32) | 0x12345678)
    w = md.philox4x32((0, 0xFFFFFFFD, 0, 3), (0, 0))
    assert md.hamiltonian_uniform(0, (1 << 32) - 3, 0) == md.uniform53(w[0], w[1])
    for a in ((1 << 32) - 1, 1 << 32, (5 << 32) + 11):  # the carry into the counter's high word
        w = md.philox4x32((14, a & 0xFFFFFFFF, a >> 32, 3), (0x90ABCDEF, 0x12345678))
        assert 0.0 < md.hamiltonian_uniform(14, a, 0x1234567890ABCDEF) == md.uniform53(w[0], w[1]) <= 1.0
    assert md.hamiltonian_uniform(14, 1 << 32, 7) != md.hamiltonian_uniform(14, 0, 7)


def test_the_constructor_checks_its_arguments_first(no_library):  # noqa: F811
    s = _System()
    ks = [_Fake(4), _Fake(4), _Fake(4)]
    H = md.HamiltonianReplicaMD
    with pytest.raises(ValueError):
        H(s, ks, [300.0, 320.0])  # lists of mismatching length
    with pytest.raises(ValueError):
        H(s, ks, [300.0, 320.0, 340.0], seeds=[1, 2])
    with pytest.raises(ValueError):
        H(s, [], [])  # R outside 1 .. 16
    with pytest.raises(ValueError):
        H(s, [_Fake(4) for _ in range(17)], [300.0] * 17)
    with pytest.raises(ValueError):
        H(s, [_Fake(4), _Fake(5)], [300.0, 300.0])  # differing particle counts
    with pytest.raises(ValueError):
        H(s, [_Fake(5), _Fake(5)], [300.0, 300.0])  # (not the system's)
    with pytest.raises(ValueError):
        H(s, [ks[0], ks[1], ks[0]], [300.0, 300.0, 300.0])  # the same kernel twice
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            H(s, ks, [300.0, bad, 300.0])  # a temperature that is not positive and finite
    # and a valid argument list -- equal temperatures are one -- does go on to the library (the fixture's refusal)
    with pytest.raises(AssertionError, match="reached the library"):
        H(s, ks, [300.0, 300.0, 300.0])


def test_the_library_exports_the_symbol_and_the_structs_have_the_kernels_sizes():
    """AgbnpMdHamiltonian: two ints, then fifteen 8-byte members; AgbnpMdHamiltonianRecord: 104 bytes without padding."""
    assert md.HAMILTONIAN_SYMBOLS == ("agbnp_md_hamiltonian_exchange",)
    lib = C.CDLL(os.path.join(ROOT, "openmm_agbnp_plugin_amd", "libagbnp_md.so"))
    for name in md.HAMILTONIAN_SYMBOLS + md.GROUP_SYMBOLS:
        getattr(lib, name)  # AttributeError if the library does not export it
    assert C.sizeof(md._HamiltonianArgs) == 8 + 15 * 8
    assert all(C.sizeof(t) == 8 for _, t in md._HamiltonianArgs._fields_[2:])
    rec = md.HAMILTONIAN_RECORD
    assert rec.itemsize == 104 == 2 * 8 + 4 * 4 + 9 * 8
    assert rec.names == ("attempt", "step", "rung", "walker_lo", "walker_hi", "accepted", "P_lo", "P_hi", "T_lo", "T_hi", "C_lo", "C_hi",
                         "kT_lo", "kT_hi", "u")
    assert [rec.fields[name][1] for name in rec.names] == [0, 8, 16, 20, 24, 28] + [32 + 8 * j for j in range(9)]
    text = open(os.path.join(ROOT, "openmm_agbnp_plugin_amd", "csrc", "md_kernels.hip")).read()
    for struct in ("AgbnpMdHamiltonian", "AgbnpMdHamiltonianRecord"):
        assert f"struct {struct} {{" in text
    assert "asm" not in text  # plain C++ only


@pytest.mark.parametrize("R", [2, 3, 16])
def test_one_hamiltonian_restated_is_the_temperature_exchange_restated(R):
    """Synthetic states whose cross words are the partner's own AGBNP energy, the Philox counter word switched to the temperature
    exchange's: over 16 attempts from 2^32 - 3 the restatement and md_restatement.exchange draw the same deviates, accept the
    same pairs and keep equal maps (walker = replica), and after every attempt every conformation sits in the same bath with the
    same velocities: what the temperature exchange does to replica r's kT and v, this one does by moving x and v to another slot."""
    n = 5
    h = hr.hamiltonian_state(n, R)
    t = mr.exchange_state(n, R, attempts=hr.ATTEMPTS)
    ladder = h["kT"].copy()
    assert np.array_equal(t["kT"], ladder)
    took = tried = 0
    for i in range(hr.ATTEMPTS):
        h = hr.energies(h, i, i % 2, one_hamiltonian=True)
        for k in range(R):  # the pairs' slots hold what the temperature exchange's replicas hold (idle slots hold sentinels)
            r = int(t["replica_at_rung"][k])
            t["last"][r, 0] = h["last"][k, 0]
        busy = [k for pair in hr.pairs(int(h["attempts"][0]), R) for k in pair]
        for k in busy:
            t["v"][int(t["replica_at_rung"][k])] = h["v"][k]
        x_before = h["x"].copy()
        h1, t1 = hr.exchange(h, hr.EXCHANGE_SEED, i % 2, counter_word=hr.TEMPERATURE_WORD), mr.exchange(t, hr.EXCHANGE_SEED)
        lo_place = mr.exchange_places(int(h["attempts"][0]), R) - h["record_base"]
        for j, (lo, hi) in enumerate(hr.pairs(int(h["attempts"][0]), R)):
            rh, rt = h1["records"][lo_place + j], t1["records"][lo_place + j]
            assert rh["u"] == rt["u"] and rh["rung"] == rt["rung"] == lo and rh["attempt"] == rt["attempt"]
            assert (rh["walker_lo"], rh["walker_hi"]) == (rt["replica_lo"], rt["replica_hi"])
            assert rh["accepted"] == rt["accepted"] and rh["accepted"] in (0, 1)
            assert hr.margin(rh)[0] > 1e-6
            tried += 1
            took += int(rh["accepted"])
        assert np.array_equal(h1["walker_at_rung"], t1["replica_at_rung"]) and np.array_equal(h1["rung_of_walker"], t1["rung_of_replica"])
        assert sorted(h1["walker_at_rung"]) == list(range(R)) and np.array_equal(h1["kT"], ladder)
        for k in busy:  # the conformation that sat in slot k
            now = int(h1["partner"][k]) if h1["partner"][k] >= 0 else k
            r = int(t["replica_at_rung"][k])
            assert h1["x"][now].tobytes() == x_before[k].tobytes()
            assert h1["kT"][now] == t1["kT"][r]
            assert h1["v"][now].tobytes() == t1["v"][r].tobytes()
        h, t = h1, t1
    assert 0 < took < tried or R == 2 and 0 < took


CASES = [(n, R) for n in (1, 256, 257) for R in (1, 2, 3, 16)]
CRAFTED = ("accept", "reject", "equal", "void0", "voidinf")  # the pairs (0,1), (2,3), ... of the even attempt at R = 16


def crafted_state(n):
    """R = 16 in front of an EVEN attempt (2^32 - 2) whose first five pairs are the certain cases of hremd_restatement.set_pair."""
    state = hr.energies(hr.hamiltonian_state(n, 16, first_attempt=hr.FIRST_ATTEMPT + 1, attempts=1), 0, 1)
    for j, kind in enumerate(CRAFTED):
        hr.set_pair(state, 1, 2 * j, kind)
    return state


def test_no_verdict_of_the_gpu_tests_inputs_hangs_on_the_last_bits():
    """The inputs of tests/test_gpu_hremd_kernels.py, judged by the restatement alone: every record's |log u - Delta| / max(1,
    |Delta|) is far above the 1e-12 below which the GPU test would not judge a verdict, both verdicts occur at every R > 1, the
    record counts are those of the place formula, and slots outside the attempt's pairs keep their sentinels."""
    for n, R in CASES:
        state = hr.hamiltonian_state(n, R)
        smallest, verdicts = np.inf, []
        for i in range(hr.ATTEMPTS):
            before = hr.energies(state, i, i % 2)
            state = hr.exchange(before, hr.EXCHANGE_SEED, i % 2)
            a = int(before["attempts"][0])
            busy = {k for pair in hr.pairs(a, R) for k in pair}
            for r in set(range(R)) - busy:
                assert state["x"][r].tobytes() == before["x"][r].tobytes() and state["v"][r].tobytes() == before["v"][r].tobytes()
                assert np.isnan(state["x"][r]).all() and state["partner"][r] == -1 and state["scale"][r] == 1.0
            assert all(state["cross"][r] == 0.0 for r in busy) and np.isnan(state["cross"][R:]).all()
            assert sorted(state["walker_at_rung"]) == list(range(R))
            assert np.array_equal(state["rung_of_walker"][state["walker_at_rung"]], np.arange(R))
        total = mr.exchange_places(hr.FIRST_ATTEMPT + hr.ATTEMPTS, R) - mr.exchange_places(hr.FIRST_ATTEMPT, R)
        assert len(state["records"]) == max(total, 1)
        for rec in state["records"][:total]:
            m, _ = hr.margin(rec)
            smallest = min(smallest, m)
            verdicts.append(int(rec["accepted"]))
        if R > 1:
            assert smallest > 1e-6, f"n {n} R {R}: a verdict hangs on {smallest:.2e}"
            assert set(verdicts) == {0, 1}, f"n {n} R {R}: verdicts {set(verdicts)}"
            print(f"n {n} R {R}: smallest margin {smallest:.2e}, {sum(verdicts)} of {len(verdicts)} accepted")
        else:
            assert set(state["records"].tobytes()) == {0xFF} and int(state["attempts"][0]) == hr.FIRST_ATTEMPT + hr.ATTEMPTS


def test_the_crafted_pairs_are_what_they_say():
    before = crafted_state(257)
    after = hr.exchange(before, hr.EXCHANGE_SEED, 1)
    recs = after["records"]
    assert len(recs) == 8 and list(recs["accepted"][:5]) == [1, 0, 1, -1, -1]
    deltas = [hr.margin(rec)[1] for rec in recs[:3]]
    assert abs(deltas[0] - 400.0) < 1e-6 and abs(deltas[1] + 400.0) < 1e-6 and abs(deltas[2]) < 1e-12
    rec = recs[2]  # in double, as the kernel forms it, the equal pair's Delta is exactly zero
    assert md.hamiltonian_delta(*(rec[key] for key in ("kT_lo", "kT_hi", "P_lo", "P_hi", "T_lo", "T_hi", "C_lo", "C_hi"))) == 0.0
    assert all(hr.margin(rec)[0] > 1e-6 for rec in recs[:3]) and all(hr.margin(rec)[0] > 1e-6 for rec in recs[5:])
    assert recs["C_lo"][3] == 0.0 and np.isinf(recs["C_hi"][4])
    assert list(after["partner"][:10]) == [1, 0, -1, -1, 5, 4, -1, -1, -1, -1]
    assert after["scale"][4] == 1.0 == after["scale"][5] and after["scale"][0] != 1.0 and np.all(after["scale"][6:10] == 1.0)
    assert after["x"][4].tobytes() == before["x"][5].tobytes() and after["v"][4].tobytes() == before["v"][5].tobytes()
    for r in range(6, 10):  # the void pairs: nothing moved, no map changed, the cross words handed back all the same
        assert after["x"][r].tobytes() == before["x"][r].tobytes() and after["walker_at_rung"][r] == r and after["cross"][r] == 0.0
        assert after["last"][r].tobytes() == before["last"][r].tobytes()
    assert list(after["walker_at_rung"][:6]) == [1, 0, 2, 3, 5, 4]
    assert after["last"][0, 1] == np.float64(np.longdouble(before["last"][1, 1]) * before["kT"][0] / before["kT"][1])


def test_a_truncated_log_keeps_the_decisions():
    """log_capacity = 12 records at R = 16: the first attempt (odd: 7 pairs) fits, the second (8 pairs) is cut after its fifth
    record; the maps go on as with a full log."""
    full, cut = hr.hamiltonian_state(257, 16), hr.hamiltonian_state(257, 16, log_capacity=12)
    for i in range(hr.ATTEMPTS):
        full = hr.exchange(hr.energies(full, i, i % 2), hr.EXCHANGE_SEED, i % 2)
        cut = hr.exchange(hr.energies(cut, i, i % 2), hr.EXCHANGE_SEED, i % 2)
    assert cut["records"][:12].tobytes() == full["records"][:12].tobytes() and set(cut["records"][12:].tobytes()) == {0xFF}
    assert cut["records"]["attempt"][11] == hr.FIRST_ATTEMPT + 1 and cut["records"]["rung"][11] == 8
    assert np.array_equal(cut["walker_at_rung"], full["walker_at_rung"]) and not np.array_equal(cut["walker_at_rung"], np.arange(16))
