"""GPU box: HamiltonianReplicaMD (openmm_agbnp_plugin_amd/md.py) end to end on trpcage (version 1): the slots
keep their contexts and baths, the conformations move.  References are twin contexts with the rung's parameters evaluated
through the host entry points (energy() / execute(), which repeat a withheld evaluation inside), as the group tests do; the
exchange decisions must be the ones the host restatements give."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.gpu_helpers import TIGHT, energy_close
from tests.gpu_helpers import five_groups as five  # noqa: F401
from tests.gpu_helpers import kernel_of as _kernel

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHARGE_LADDER = (1.0, 0.95, 0.9, 0.85)


def _scaled(s, q):
    radius, gamma, alpha, charge, ish = s.params()
    return radius, gamma, alpha, charge * q, ish


def _driver(s, temperatures, charges=None, **kw):
    from openmm_agbnp_plugin_amd.md import HamiltonianReplicaMD
    charges = [1.0] * len(temperatures) if charges is None else charges
    ks = [_kernel(_scaled(s, q)) for q in charges]
    rep = HamiltonianReplicaMD(s, ks, temperatures, **kw)
    rep.settle()
    return rep, ks


def _start(rep):
    rep.forces()
    assert not rep.finish().any()


def _tether_sum(rep, part):
    """The sequential sum of every slot's tether partials, as the deciding thread takes it."""
    parts = rep.core.parts[part].cpu().numpy()
    out = np.zeros(rep.R)
    for b in range(parts.shape[1]):
        out = out + parts[:, b]
    return out


def _judge(rec, skipped):
    from openmm_agbnp_plugin_amd.md import hamiltonian_delta
    delta = hamiltonian_delta(*(rec[key] for key in ("kT_lo", "kT_hi", "P_lo", "P_hi", "T_lo", "T_hi", "C_lo", "C_hi")))
    if abs(np.log(rec["u"]) - delta) < 1e-12 * max(1.0, abs(delta)):
        skipped.append(rec)
    else:
        assert int(rec["accepted"]) == int(np.log(rec["u"]) <= delta), f"verdict {rec['accepted']} for Delta {delta}, u {rec['u']}"
    return delta


def test_one_hamiltonian_is_temperature_exchange(gpu_required, systems, five):
    """R = 4 contexts with the same parameters on a ladder of ratio 1.03 from 300 K, 60 attempts 10 steps apart.  Every record: P
    is the rung's logged potential of the step just finished, bit for bit (the refresh behind an attempt is overwritten by the
    steps that follow, so every attempt sees a step); T the sequential sum of the partial buffer the last back half read; u the
    host's; hamiltonian_delta of the record agrees with exchange_delta(kT_lo, kT_hi, P_lo, P_hi) within 2 TIGHT max(1, 1e-3 |A|) /
    kT_lo -- the project's energy bound on the two cross words over the temperature; the verdict recomputed (records with
    |log u - Delta| < 1e-12 max(1, |Delta|) are not judged: fewer than 1 %).  The maps replayed from the log are the device's and
    permutations after every attempt; both verdicts occur; nothing is withheld."""
    pytest.importorskip("torch")
    from openmm_agbnp_plugin_amd.md import KB, exchange_delta, hamiltonian_uniform
    s = systems("trpcage")
    ladder = [300.0 * 1.03 ** k for k in range(4)]
    kT_ladder = np.array([KB * t for t in ladder])
    seed = 0x1234567890ABCDEF
    rep, _ = _driver(s, ladder, seeds=[21, 22, 23, 24], exchange_seed=seed)
    _start(rep)
    attempts, sitting, skipped, log_seen, worst = 60, np.arange(4), [], 0, 0.0
    for a in range(attempts):
        # (a chunk of 10 steps: its last back half read parts[(10 - 1) % 2], which the attempt's refresh -- parts[0] -- leaves alone)
        assert not rep.run(10, "langevin", exchange_every=10, check_every=10).any()
        tether = _tether_sum(rep, 1)
        log = rep.exchange_log()
        pe, _ = rep.energies()
        assert pe.shape == (4, 10 * (a + 1))
        for rec in log[log_seen:]:
            k = int(rec["rung"])
            assert int(rec["attempt"]) == a and k % 2 == a % 2 and 0 <= k < 3 and int(rec["step"]) == 10 * (a + 1)
            assert (sitting[k], sitting[k + 1]) == (rec["walker_lo"], rec["walker_hi"])
            assert rec["P_lo"] == pe[k, -1] and rec["P_hi"] == pe[k + 1, -1]
            assert rec["T_lo"] == tether[k] and rec["T_hi"] == tether[k + 1]
            assert rec["kT_lo"] == kT_ladder[k] and rec["kT_hi"] == kT_ladder[k + 1]
            assert rec["u"] == hamiltonian_uniform(k, a, seed)
            delta = _judge(rec, skipped)
            agbnp = max(abs(rec["C_lo"]), abs(rec["C_hi"]))
            bound = 2.0 * TIGHT * max(1.0, 1e-3 * agbnp) / rec["kT_lo"]
            off = abs(delta - exchange_delta(rec["kT_lo"], rec["kT_hi"], rec["P_lo"], rec["P_hi"]))
            worst = max(worst, off / bound)
            assert off < bound, f"Delta {delta} is {off:.3e} off the temperature exchange's (allowed {bound:.3e})"
            assert rec["accepted"] in (0, 1)
            if rec["accepted"] == 1:
                sitting[k], sitting[k + 1] = sitting[k + 1], sitting[k]
        log_seen = len(log)
        walkers = rep.walkers()
        assert sorted(walkers) == [0, 1, 2, 3] and np.array_equal(walkers, sitting)
        assert np.array_equal(rep.rung_of_walker.cpu().numpy()[walkers], np.arange(4))
        assert np.array_equal(rep.kT.cpu().numpy(), kT_ladder)  # the baths never move
    assert log_seen == (attempts // 2) * 2 + (attempts // 2) * 1
    assert len(skipped) < 0.01 * log_seen
    accepted = int((log["accepted"] == 1).sum())
    print(f"{accepted} of {log_seen} exchanges accepted; acceptance per pair {rep.acceptance()}; Delta off by {worst:.2e} of its bound")
    assert 0 < accepted < log_seen
    acc = rep.acceptance()
    for k in range(3):
        sel = log["rung"] == k
        assert acc[k] == (log["accepted"][sel] == 1).sum() / sel.sum()


def test_a_charge_ladder_against_twin_contexts(gpu_required, systems, five):
    """R = 4 at 300 K, charges scaled by 1, 0.95, 0.9, 0.85; 20 attempts made by hand: run(10, exchange_every=0), read x,
    exchange().  Every record's cross words are the twin context's energy of THAT rung's parameters at the PARTNER's conformation
    as read before the attempt, and P - T the rung's own; afterwards x and v of an accepted pair are the other's (bit for bit,
    times `scale` to 1e-15 relative) and every other slot is unchanged bit for bit; after the refresh last[k][0] and frc[k] are
    tethers + the twin's energy and forces of rung k at what it now holds, and every member reads a group of R."""
    pytest.importorskip("torch")
    s = systems("trpcage")
    R = 4
    rep, ks = _driver(s, [300.0] * R, charges=CHARGE_LADDER, seeds=[61, 62, 63, 64], exchange_seed=5)
    twins = [_kernel(_scaled(s, q)) for q in CHARGE_LADDER]
    x0 = rep.x0.cpu().numpy()
    _start(rep)
    skipped, seen, took = [], 0, 0
    for a in range(20):
        assert not rep.run(10, "langevin", exchange_every=0, check_every=10).any()
        x, v = rep.x.cpu().numpy(), rep.v.cpu().numpy()
        own = [twins[k].energy(x[k]) for k in range(R)]
        rep.exchange()
        assert not rep.finish().any()
        log = rep.exchange_log()
        scale, partner = rep.scale.cpu().numpy(), rep.partner.cpu().numpy()
        x1, v1 = rep.x.cpu().numpy(), rep.v.cpu().numpy()
        assert len(log) - seen == len(range(a % 2, R - 1, 2))
        for rec in log[seen:]:
            lo, hi = int(rec["rung"]), int(rec["rung"]) + 1
            assert int(rec["attempt"]) == a and rec["accepted"] in (0, 1)
            energy_close(rec["C_lo"], twins[lo].energy(x[hi]))
            energy_close(rec["C_hi"], twins[hi].energy(x[lo]))
            energy_close(rec["P_lo"] - rec["T_lo"], own[lo])
            energy_close(rec["P_hi"] - rec["T_hi"], own[hi])
            _judge(rec, skipped)
            assert (partner[lo], partner[hi]) == ((hi, lo) if rec["accepted"] == 1 else (-1, -1))
            took += int(rec["accepted"] == 1)
        seen = len(log)
        for k in range(R):
            q = int(partner[k])
            if q < 0:
                assert scale[k] == 1.0 and np.array_equal(x1[k], x[k]) and np.array_equal(v1[k], v[k]), f"slot {k} did not move and changed"
            else:
                assert np.array_equal(x1[k], x[q]), f"x[{k}] is not the old x[{q}]"
                want = v[q] * scale[k]
                assert np.all(np.abs(v1[k] - want) <= 1e-15 * np.abs(want))
        # the refresh: rung k's Hamiltonian at the conformation slot k now holds
        last, frc, tether = rep.last.cpu().numpy(), rep.frc.cpu().numpy(), _tether_sum(rep, 0)
        for k in range(R):
            f = -rep.k * (x1[k] - x0)
            e = twins[k].execute(x1[k], f)
            energy_close(last[k, 0], tether[k] + e)
            energy_close(tether[k], 0.5 * rep.k * ((x1[k] - x0) ** 2).sum())
            assert np.abs(frc[k] - f).max() < TIGHT, f"frc[{k}] differs by {np.abs(frc[k] - f).max():.3e}"
        assert [int(k.scalar("group_members")) for k in ks] == [R] * R
        assert sorted(rep.walkers()) == list(range(R))
    assert len(skipped) < 0.01 * seen or len(skipped) == 0
    print(f"{took} of {seen} exchanges accepted; acceptance per pair {rep.acceptance()}")
    assert took > 0


def test_a_certain_exchange_across_a_jump(gpu_required, systems, five):
    """R = 2, one Hamiltonian, both at 300 K, slot 1's conformation shifted rigidly by 0.1 nm (the displacement with which
    test_a_withheld_member_is_reported_as_that_member makes a jump): the tether energies differ widely, the baths do not, so Delta
    is 0 up to the bound of the first test and the attempt is accepted (log u <= 0; u of this seed is not within 1e-7 of 1).  finish()
    reads zeros behind the attempt -- every cross evaluation sits 0.1 nm from the member's last, and so does every refresh
    evaluation after the swap: the hints are placed -- the cross words are the partner's own AGBNP energy (translation
    invariance), x is swapped bit for bit, and the steps that follow are complete."""
    pytest.importorskip("torch")
    from openmm_agbnp_plugin_amd.md import hamiltonian_delta
    s = systems("trpcage")
    rep, _ = _driver(s, [300.0, 300.0], seeds=[71, 72], exchange_seed=3)
    rep.x[1, :, 0].add_(0.1)
    rep.forces()  # (slot 1 jumped: this evaluation may be withheld for it, the next one is not)
    rep.finish()
    _start(rep)
    x, last = rep.x.cpu().numpy(), rep.last.cpu().numpy()
    tether = _tether_sum(rep, 0)
    rep.exchange()
    assert list(rep.finish()) == [0, 0]
    log = rep.exchange_log()
    assert len(log) == 1
    rec = log[0]
    assert rec["P_lo"] == last[0, 0] and rec["P_hi"] == last[1, 0] and rec["T_lo"] == tether[0] and rec["T_hi"] == tether[1]
    energy_close(rec["C_lo"], rec["P_hi"] - rec["T_hi"])
    energy_close(rec["C_hi"], rec["P_lo"] - rec["T_lo"])
    delta = hamiltonian_delta(*(rec[key] for key in ("kT_lo", "kT_hi", "P_lo", "P_hi", "T_lo", "T_hi", "C_lo", "C_hi")))
    assert abs(delta) < 2.0 * TIGHT * max(1.0, 1e-3 * abs(rec["C_lo"])) / rec["kT_lo"]
    assert rec["accepted"] == 1 and list(rep.walkers()) == [1, 0] and list(rep.partner.cpu().numpy()) == [1, 0]
    x1 = rep.x.cpu().numpy()
    assert np.array_equal(x1[0], x[1]) and np.array_equal(x1[1], x[0])
    assert list(rep.run(10, "verlet", check_every=10)) == [0, 0]
    # the next attempt (odd) has no pair at R = 2: only the counter moves
    x2, v2 = rep.x.cpu().numpy(), rep.v.cpu().numpy()
    rep.exchange()
    assert len(rep.exchange_log()) == 1 and int(rep.attempts.item()) == 2
    assert np.array_equal(rep.x.cpu().numpy(), x2) and np.array_equal(rep.v.cpu().numpy(), v2) and list(rep.finish()) == [0, 0]


def test_a_steady_run_between_attempts_rewrites_nothing(gpu_required, systems, five):
    """scalar 21 (group_block_writes) of every member stands still over 100 steps without an attempt and moves only across
    exchange(): the cross round hands a paired member its partner's position buffer, and the engine keeps one argument block per
    parity of its evaluations, so the block comes back to the member's own buffer at the first evaluation of that parity behind
    the attempt -- the refresh or the first step.  Two steps behind an attempt the run is steady again."""
    pytest.importorskip("torch")
    R = 4
    rep, ks = _driver(systems("trpcage"), [300.0] * R, charges=CHARGE_LADDER)
    writes = lambda: [int(k.scalar("group_block_writes")) for k in ks]  # noqa: E731
    _start(rep)
    assert not rep.run(2, "langevin", check_every=2).any()
    w0 = writes()
    assert not rep.run(100, "langevin", check_every=50).any()
    assert writes() == w0
    rep.exchange()  # (attempt 0 pairs (0, 1) and (2, 3): every member's pointer moves)
    assert not rep.run(2, "langevin", check_every=2).any()
    w1 = writes()
    assert [b - a for a, b in zip(w0, w1)] == [2] * R  # there and back
    assert not rep.run(100, "langevin", check_every=50).any()
    assert writes() == w1
    assert [int(k.scalar("group_members")) for k in ks] == [R] * R
    rep.exchange()  # (attempt 1 pairs (1, 2): slots 0 and 3 sit out)
    assert not rep.run(2, "langevin", check_every=2).any()
    assert [b - a for a, b in zip(w1, writes())] == [0, 2, 2, 0]


def test_the_example_script_runs(gpu_required):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "hremd_benchmark.py"), "trpcage", "4", "1000", "50"],
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "ns/day aggregate" in out.stdout and "acceptance" in out.stdout
    assert "WARNING" not in out.stdout
