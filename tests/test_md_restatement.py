"""The CPU restatement of libagbnp_md.so's entry points (tests/md_restatement.py) against itself, so that the reference is known
good before tests/test_gpu_md_kernels.py judges a kernel by it.  Nothing here needs a device."""
import numpy as np
import pytest

from openmm_agbnp_plugin_amd import md
from tests import md_restatement as mr
from tests.md_kernel_harness import assert_same_state, same_bits

LD = np.longdouble


@pytest.mark.parametrize("kind", [mr.LANGEVIN, mr.VERLET])
def test_mid_is_post_then_pre(kind):
    """Three `mid` launches with the partial buffers alternating, each against `post` then `pre` from the same state: every word
    bit for bit (300 atoms: two blocks; three replicas with the step words 5, 7 and 2^32 + 3 against a log of 8)."""
    state = mr.synthetic_state(300, 3)
    y0 = mr.standin_anchor(state)
    state = mr.pre(mr.tethers(state, 0), kind, 0)
    for j in range(3):
        state = mr.evaluated(state, y0)
        old, new = j % 2, (j + 1) % 2
        one = mr.mid(state, kind, old, new)
        two = mr.pre(mr.post(state, old), kind, new)
        assert_same_state(one, two)
        assert not same_bits(one["x"], state["x"]) and list(one["step"]) == [s + 1 for s in state["step"]]
        state = one
    # the log of 8: replica 0 wrote slots 5, 6, 7; replica 1 slot 7 and was refused twice; replica 2 never wrote
    written = ~np.isnan(state["log_pe"])
    assert list(np.flatnonzero(written)) == [5, 6, 7, 8 + 7]
    assert same_bits(np.isnan(state["log_ke"]), ~written)


def test_a_function_leaves_its_argument_alone():
    state = mr.evaluated(mr.synthetic_state(5, 2), mr.standin_anchor(mr.synthetic_state(5, 2)))
    keep = mr.copy_state(state)
    mr.tethers(state, 1), mr.pre(state, mr.LANGEVIN, 0), mr.mid(state, mr.VERLET, 0), mr.post(state, 0)
    assert_same_state(state, keep)


def test_the_tether_energy_is_the_tether_forces_potential():
    """Central differences of the summed partials on three atoms (first and last of block 0, last of all), every component:
    relative 1e-6 (the energy is quadratic, so the difference quotient is exact up to rounding)."""
    state = mr.synthetic_state(300, 2)
    f = mr.tethers(state, 0)["f"]
    h = 1e-4
    for r in range(2):
        for i in (0, 255, 299):
            for d in range(3):
                e = []
                for sign in (1.0, -1.0):
                    moved = mr.copy_state(state)
                    moved["x"][r, i, d] += sign * h
                    e.append(mr.tethers(moved, 0)["parts"][0][r].astype(LD).sum())
                slope = float((e[0] - e[1]) / (2 * LD(h)))
                assert abs(slope + f[r, i, d]) <= 1e-6 * abs(f[r, i, d]), (r, i, d, slope, f[r, i, d])


def test_verlet_steps_of_the_tethers_conserve_energy():
    """200 restated velocity-Verlet steps with no force but the tethers.  Velocity Verlet conserves, for every harmonic degree
    of freedom, E~ = K + (1 - a) U exactly, a = k dt^2 / (4 m); so E(t) - E(0) = a (U(t) - U(0)), with U <= E~ / (1 - a) and
    E~ <= E(0): |E(t) - E(0)| <= sum over atoms of a_i / (1 - a_i) E_i(0).  With k = 2e4, dt = 1 fs that is 0.5 % of a
    hydrogen's energy, 0.04 % of a heavy atom's; storing doubles adds rounding of 200 x 2^-53 relative, taken as 1e-12."""
    n, R, steps = 7, 2, 200
    state = mr.synthetic_state(n, R, capacity=steps, steps=(0, 0))
    state["x"] = state["x0"][None] + 0.02 * np.sin(37.0 * state["x0"][None] + np.arange(R)[:, None, None])
    k, dt, m = state["k"], state["dt"], state["mass"]
    e_atom = 0.5 * k * ((state["x"] - state["x0"][None]) ** 2).sum(axis=2) + 0.5 * m[None] * (state["v"] ** 2).sum(axis=2)
    a = k * dt * dt / (4.0 * m)
    bound = (a / (1.0 - a))[None] * e_atom
    bound = bound.sum(axis=1) + 1e-12 * e_atom.sum(axis=1)
    state = mr.pre(mr.tethers(state, 0), mr.VERLET, 0)
    for j in range(steps):
        state = mr.mid(state, mr.VERLET, j % 2) if j + 1 < steps else mr.post(state, j % 2)
    assert list(state["step"]) == [steps] * R
    total = (state["log_pe"] + state["log_ke"])[:R * steps].reshape(R, steps)
    for r in range(R):
        worst = np.abs(total[r] - e_atom[r].sum()).max()
        print(f"replica {r}: E(0) {e_atom[r].sum():.4f}  worst |E(t) - E(0)| {worst:.3e}  bound {bound[r]:.3e} kJ/mol")
        assert worst <= bound[r]
        assert worst > 0.01 * bound[r]  # (the bound is of the error's own order: the energies do move)


def _exchange_run(R, **kw):
    state = mr.exchange_state(1, R, **kw)
    energies = mr.exchange_energies(R)
    for u in energies:
        state["last"][:, 0] = u
        state = mr.exchange(state, mr.EXCHANGE_SEED)
    return state


@pytest.mark.parametrize("R,records,accepted", [(2, 32, 27), (3, 64, 54), (5, 128, 101), (16, 480, 378)])
def test_the_exchange_inputs_are_fit_for_purpose(R, records, accepted):
    """The inputs of the GPU exchange tests through the restatement, every record recomputed with md.exchange_delta /
    md.exchange_uniform in double: no verdict hangs on the last bits (|log u - Delta| > 1e-6 max(1, |Delta|) for every record),
    so the GPU test judges every record; both verdicts occur; the number of records is the place formula's."""
    state = _exchange_run(R)
    log = state["records"]
    first, a_end = mr.FIRST_ATTEMPT, mr.FIRST_ATTEMPT + 64
    assert int(state["attempts"][0]) == a_end and first < (1 << 32) < a_end
    assert len(log) == mr.exchange_places(a_end, R) - mr.exchange_places(first, R) == records
    assert sum(len(range(a & 1, R - 1, 2)) for a in range(first, a_end)) == records
    margins = []
    for rec in log:
        a, k = int(rec["attempt"]), int(rec["rung"])
        assert first <= a < a_end and k % 2 == a % 2 and rec["u"] == md.exchange_uniform(k, a, mr.EXCHANGE_SEED)
        assert rec["step"] == 1000 + 7 * rec["replica_lo"]
        delta = md.exchange_delta(rec["kT_lo"], rec["kT_hi"], rec["U_lo"], rec["U_hi"])
        margins.append(abs(np.log(rec["u"]) - delta) / max(1.0, abs(delta)))
        assert bool(rec["accepted"]) == bool(np.log(rec["u"]) <= delta)
    assert list(log["attempt"]) == sorted(log["attempt"])
    took = int(log["accepted"].sum())
    print(f"R = {R}: {took} of {len(log)} accepted, smallest margin {min(margins):.2e}")
    assert min(margins) > 1e-6
    assert 0 < took < len(log)
    assert took == accepted
    assert sorted(state["rung_of_replica"]) == list(range(R))
    assert np.array_equal(state["replica_at_rung"][state["rung_of_replica"]], np.arange(R))
    assert np.array_equal(state["kT"], (md.KB * 300.0 * 1.05 ** np.arange(R))[state["rung_of_replica"]])


def test_the_drivers_log_places_are_the_restatements():
    """md.exchange_places against the restatement's own copy of the formula: R = 1 (no pair), 2 (none at odd attempts), odd and
    even R up to a full group; the first attempts and those around 2^32, where the attempt number outgrows a 32-bit word."""
    for R in (1, 2, 3, 5, 16):
        for a in list(range(10)) + list(range((1 << 32) - 3, (1 << 32) + 4)):
            assert md.exchange_places(a, R) == mr.exchange_places(a, R), (a, R)


def test_a_truncated_exchange_log_keeps_the_decisions():
    """log_capacity 40 records over a buffer of 160 at R = 5: the first 40 records are the full run's, the rest stays 0xFF, and
    temperatures and rungs end where the full run's end."""
    full, cut = _exchange_run(5), _exchange_run(5, log_capacity=40, buffer=160)
    assert same_bits(cut["records"][:40], full["records"][:40])
    assert set(cut["records"][40:].tobytes()) == {0xFF}
    for key in ("kT", "rung_of_replica", "replica_at_rung", "attempts", "v"):
        assert same_bits(cut[key], full[key]), key


def test_one_replica_has_nobody_to_exchange_with():
    state = mr.exchange_state(3, 1)
    state["scale"][:] = 1.0
    state["last"][:, 0] = -1000.0
    after = mr.exchange(state, mr.EXCHANGE_SEED)
    assert int(after["attempts"][0]) == mr.FIRST_ATTEMPT + 1
    after["attempts"][0] = mr.FIRST_ATTEMPT
    assert_same_state(after, state)
