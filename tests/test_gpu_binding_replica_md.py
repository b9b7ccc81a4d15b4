"""GPU box: BindingReplicaMD (openmm_agbnp_plugin_amd/md.py) -- R replicas of trpcage with the ligand 0 .. 15 on a
lambda ladder, advanced by the group forms of the integrator kernels around agbnp_hip_binding_execute_group, with lambda
exchanges decided on the device from the u words the steps' own last evaluation left.  Every exchange decision must be the one
the host restatement md.lambda_delta gives from the record; what the evaluations add is judged against the CPU restatement of
tests/binding_restatement.py within the tolerances of tests/test_gpu_binding.py (TIGHT per member evaluation and the weights of
the combination)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import openmm_agbnp_plugin_amd as P
from openmm_agbnp_plugin_amd import md as MD
from tests.binding_restatement import BindingRestatement, combine
from tests.gpu_helpers import TIGHT
from tests.gpu_helpers import five_groups as five  # noqa: F401
from tests.test_gpu_binding import _binding

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIGAND = list(range(16))
LADDER = [0.0, 1.0 / 3.0, 2.0 / 3.0, 1.0]


def _driver(s, ladder=LADDER, temperatures=300.0, **kw):
    bindings = [_binding(s, LIGAND) for _ in ladder]
    rep = MD.BindingReplicaMD(s, bindings, ladder, temperatures, **kw)
    rep.settle()
    return rep, bindings


def _check_maps(rep, log):
    """Both maps are inverse permutations, and they and lambdas() are what the accepted records, replayed in order, leave."""
    R = rep.R
    at, lam = list(range(R)), list(rep.lambda_ladder)
    for rec in log:
        k, lo, hi = int(rec["rung"]), int(rec["replica_lo"]), int(rec["replica_hi"])
        assert (at[k], at[k + 1]) == (lo, hi)
        assert rec["lambda_lo"] == lam[lo] == rep.lambda_ladder[k] and rec["lambda_hi"] == lam[hi] == rep.lambda_ladder[k + 1]
        if rec["accepted"] == 1:
            at[k], at[k + 1] = hi, lo
            lam[lo], lam[hi] = lam[hi], lam[lo]
    rungs = rep.rungs()
    assert sorted(rungs) == list(range(R))
    assert list(rep.replica_at_rung.cpu().numpy()) == at and [at[k] for k in rungs] == list(range(R))
    assert list(rep.lambdas()) == lam and list(rep.lambdas()[at]) == list(rep.lambda_ladder)


def test_invariants_of_a_run(gpu_required, systems, five):
    """R = 4, lambda = 0, 1/3, 2/3, 1, 300 K: 40 Langevin steps after settle() with an attempt every 10.  Every record's verdict is
    log(uniform) <= lambda_delta(...) recomputed from the record, its deviate is lambda_uniform's, the maps and lambdas() follow
    from the accepted records, nothing is withheld, no pair is void, and no u word is left behind."""
    pytest.importorskip("torch")
    s = systems("trpcage")
    rep, bindings = _driver(s, exchange_seed=11)
    rep.forces()
    assert not rep.finish().any()
    assert not rep.u.any().item()  # (settle() and forces() pass no u pointer)
    missed = rep.run(40, "langevin", exchange_every=10, check_every=20)
    assert not missed.any() and all(b.withheld() == [] for b in bindings)
    log = rep.exchange_log()
    assert log.dtype == MD.LAMBDA_RECORD and len(log) == MD.exchange_places(4, 4) == 2 + 1 + 2 + 1
    assert list(log["attempt"]) == [0, 0, 1, 2, 2, 3] and list(log["rung"]) == [0, 2, 1, 0, 2, 1]
    assert int(rep.attempts.item()) == 4
    kT = MD.KB * 300.0
    for rec in log:
        assert rec["accepted"] in (0, 1), "a void pair"
        assert rec["step"] == 10 * (rec["attempt"] + 1) and rec["kT_lo"] == rec["kT_hi"] == kT
        assert rec["uniform"] == MD.lambda_uniform(rec["rung"], rec["attempt"], 11)
        delta = MD.lambda_delta(rec["lambda_lo"], rec["lambda_hi"], rec["kT_lo"], rec["kT_hi"], rec["u_lo"], rec["u_hi"])
        margin = abs(np.log(rec["uniform"]) - delta)
        print(f"attempt {rec['attempt']} rungs {rec['rung']}<->{rec['rung'] + 1}: u {rec['u_lo']:.4f} {rec['u_hi']:.4f}  Delta {delta:+.4f}  "
              f"log(uniform) {np.log(rec['uniform']):+.4f}  accepted {rec['accepted']}")
        if margin > 1e-9 * max(1.0, abs(delta)):
            assert rec["accepted"] == int(np.log(rec["uniform"]) <= delta)
        assert 300.0 < rec["u_lo"] < 600.0 and 300.0 < rec["u_hi"] < 600.0  # (u of trpcage 0 .. 15 is some 440 kJ/mol)
    assert set(log["accepted"]) == {0, 1}  # (both verdicts occur: the ladder's thirds of lambda give |Delta| of several units)
    _check_maps(rep, log)
    acc = rep.acceptance()
    assert acc.shape == (3,) and np.all((acc >= 0.0) & (acc <= 1.0))
    assert not rep.u.any().item()  # every u word went back to zero
    pot, kin = rep.energies()
    assert pot.shape == kin.shape == (4, 40) and np.isfinite(pot).all() and np.isfinite(kin).all()
    assert rep.steps_done == 40 and list(rep.counter.cpu().numpy()) == [40] * 4


def test_u_and_the_refresh_are_the_restatements(gpu_required, systems, five):
    """Ten steps and one attempt (even: the pairs (0,1), (2,3) read all four u words).  No position moves in an attempt, so x[r]
    are the positions the tenth evaluation saw: the recorded u is the restatement's at x[r], and the refresh behind the attempt
    left tethers + E_lambda and tethers + F_lambda at the lambda replica r holds NOW."""
    pytest.importorskip("torch")
    s = systems("trpcage")
    rep, bindings = _driver(s, exchange_seed=3, temperatures=[300.0, 310.0, 320.0, 330.0])
    rep.forces()
    assert not rep.finish().any()
    assert not rep.run(10, "langevin", exchange_every=10, check_every=10).any()
    log = rep.exchange_log()
    assert len(log) == 2 and set(log["accepted"]) <= {0, 1}
    _check_maps(rep, log)
    lam = rep.lambdas()
    x, frc, last = rep.x.cpu().numpy(), rep.frc.cpu().numpy(), rep.last.cpu().numpy()
    ref = BindingRestatement(s.params(), LIGAND)
    u_seen = {}
    for rec in log:
        u_seen[int(rec["replica_lo"])], u_seen[int(rec["replica_hi"])] = rec["u_lo"], rec["u_hi"]
        assert rec["kT_lo"] == MD.KB * (300.0 + 10.0 * rec["replica_lo"]) and rec["kT_hi"] == MD.KB * (300.0 + 10.0 * rec["replica_hi"])
    for r in range(4):
        energies, f_rl, f_own = ref.evaluate(x[r])
        e_ref, u_ref, f_ref = combine(energies, f_rl, f_own, lam[r])
        unit = max(1.0, 1e-3 * max(abs(w) for w in energies))
        d = x[r] - s.pos
        tether_e, tether_f = 0.5 * rep.k * float((d * d).sum()), -rep.k * d
        du, de = abs(u_seen[r] - u_ref), abs(last[r, 0] - tether_e - e_ref)
        df = float(np.abs(frc[r] - tether_f - f_ref).max())
        print(f"replica {r} lambda {lam[r]:.3f}: |du| {du:.2e}  |dE_lam| {de:.2e}  max|dF| {df:.2e}  (scale {unit:.3f})")
        assert du < 3.0 * TIGHT * unit
        # (the tethers are formed here and on the device in double: a sum of 3 N = 816 terms and a product, 1e-12 relative at most)
        assert de < TIGHT * (abs(lam[r]) + 2.0 * abs(1.0 - lam[r])) * unit + 1e-12 * abs(tether_e)
        assert df < TIGHT * (abs(lam[r]) + abs(1.0 - lam[r])) + 1e-12 * float(np.abs(tether_f).max())


def test_steps_without_an_attempt_pass_no_u_pointer_and_minimise_works(gpu_required, systems, five):
    """run() without exchanges, forces() and minimise() leave the u words alone (a u pointer is passed by the last evaluation in
    front of an attempt alone); FIRE runs on E_lambda through the same evaluation; R = 1 is a ladder too."""
    pytest.importorskip("torch")
    s = systems("trpcage")
    rep, bindings = _driver(s, ladder=[0.25, 0.75])
    rec = rep.minimise(max_iterations=6, check_every=3)
    assert len(rec) == 2 and not rec["withheld"].any() and not rec["voids"].any()
    assert np.isfinite(rec["energy"]).all() and np.isfinite(rec["fmax"]).all() and (rec["iterations"] >= 1).all()
    assert not rep.run(5, "langevin", check_every=5).any()
    assert not rep.run(4, "verlet", exchange_every=0).any()
    assert not rep.u.any().item() and int(rep.attempts.item()) == 0 and len(rep.exchange_log()) == 0
    assert list(rep.lambdas()) == [0.25, 0.75] and list(rep.rungs()) == [0, 1]
    # exchange() by hand finds no u word: the pair is void, nothing swaps
    rep.exchange()
    log = rep.exchange_log()
    assert len(log) == 1 and log["accepted"][0] == -1 and list(rep.lambdas()) == [0.25, 0.75]
    assert not rep.finish().any()
    one, _ = _driver(s, ladder=[0.5])
    assert not one.run(4, "langevin", exchange_every=2).any()
    assert int(one.attempts.item()) == 2 and len(one.exchange_log()) == 0 and list(one.lambdas()) == [0.5]


def test_the_example_runs(gpu_required, systems, five):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "bedam_benchmark.py"), "trpcage", "0", "15", "4", "200", "20"],
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    print(out.stdout)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "acceptance k<->k+1" in out.stdout and "mean u per rung" in out.stdout and "ms/step" in out.stdout
    assert "WARNING" not in out.stdout and "void pairs: 0 of" in out.stdout
