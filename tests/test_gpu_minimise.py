"""GPU box: minimise() of the three MD drivers (openmm_agbnp_plugin_amd/md.py) end to end on trpcage (version
1, k_tether 2e4, the defaults of minimise()).  The reference is the same FIRE on the CPU -- tests/fire_restatement.minimise, the
restatement of the kernels -- around the CPU oracle plus tethers; it needs about 170 iterations from the file's coordinates and
is run once for the module.  Two such CPU runs from starts 0.005 nm apart end within 2e-5 kJ/mol and 2.2e-5 nm of one another:
the bounds here, 1e-3 kJ/mol and 1e-3 nm, are fifty times that."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import fire_restatement as fr
from tests.gpu_helpers import TIGHT, energy_close
from tests.gpu_helpers import five_groups as five  # noqa: F401
from tests.gpu_helpers import kernel_of as _kernel

pytestmark = pytest.mark.gpu
K_TETHER, TOLERANCE, CAP = 2.0e4, 0.3, 400
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _scaled(s, q):
    radius, gamma, alpha, charge, ish = s.params()
    return radius, gamma, alpha, charge * q, ish


def _oracle(s, q=1.0):
    from oracle import Oracle
    return Oracle(*_scaled(s, q), version=1)


def _total(oracle, x, x0):
    """Tethers + AGBNP on the CPU: (energy, forces)."""
    e, f = oracle.execute(x)
    d = x - x0
    return float(e) + 0.5 * K_TETHER * float((d * d).sum()), np.asarray(f) - K_TETHER * d


def _fmax(f):
    return float(np.sqrt((f * f).sum(axis=1)).max())


@pytest.fixture(scope="module")
def reference(systems):
    s = systems("trpcage")
    oracle = _oracle(s)
    mass = np.where(s.ishydrogen == 1, 1.008, 12.0)
    x0 = np.ascontiguousarray(s.pos, dtype=np.float64)

    def evaluate(x):
        e, f = oracle.execute(x)
        return float(e), np.asarray(f)

    out = fr.minimise(evaluate, x0, x0, mass, K_TETHER, tolerance=TOLERANCE, max_iterations=CAP)
    print(f"CPU reference: {out['iterations']} iterations, E {out['log_e'][0]:.4f} -> {out['energy']:.6f} kJ/mol, fmax {out['log_fmax'][0]:.1f} -> "
          f"{out['fmax']:.3f}, {out['capped']} iterations with a capped atom")
    assert out["converged"] and out["capped"] > 0
    return out


def _judge_final(what, s, oracle, x, record):
    """The force criterion and the returned energy at the final positions, recomputed on the CPU."""
    e, f = _total(oracle, x, np.asarray(s.pos, dtype=np.float64))
    print(f"{what}: {int(record['iterations'])} iterations, E {record['energy']:.6f} (oracle {e:.6f}), fmax {record['fmax']:.4f} (oracle {_fmax(f):.4f})")
    assert record["converged"] == 1 and 0 < record["iterations"] <= CAP
    assert record["voids"] == 0 and record["withheld"] == 0
    assert _fmax(f) < TOLERANCE * (1.0 + 1e-6)
    assert abs(record["fmax"] - _fmax(f)) < np.sqrt(3.0) * TIGHT  # (a norm of three components, each within the project's force bound)
    energy_close(record["energy"], e)


def test_device_md_minimises_as_the_cpu_reference(gpu_required, systems, five, reference):
    torch = pytest.importorskip("torch")
    from openmm_agbnp_plugin_amd.md import DeviceMD
    s = systems("trpcage")
    k = _kernel(s.params())
    md = DeviceMD(s, k, k_tether=K_TETHER, dt=0.001, temperature=300.0, seed=3)
    md.settle()
    v0, pe0, ke0 = md.v.clone(), md.log_pe.clone(), md.log_ke.clone()
    checks = []
    out = md.minimise(tolerance=TOLERANCE, max_iterations=CAP, on_check=lambda converged: checks.append(converged.copy()))
    assert out.shape == (1,) and out.dtype.names == ("iterations", "converged", "fmax", "energy", "voids", "withheld")
    x = md.x.cpu().numpy()
    _judge_final("DeviceMD", s, _oracle(s), x, out[0])
    de, dx = abs(out[0]["energy"] - reference["energy"]), np.abs(x - reference["x"]).max()
    print(f"against the CPU run ({reference['iterations']} iterations): |dE| {de:.2e} kJ/mol  |dx| {dx:.2e} nm")
    assert de < 1e-3 and dx < 1e-3
    assert len(checks) == -(-int(out[0]["iterations"]) // 50) and checks[-1].all()
    # the logs: one slot per judged evaluation, the first the start's, the last the returned one's
    log_e, log_fmax = md.core.minimisation_log()
    assert log_e.shape == (1, int(out[0]["iterations"]))
    energy_close(log_e[0, 0], reference["log_e"][0])
    energy_close(log_e[0, -1], out[0]["energy"])
    assert abs(log_fmax[0, 0] - reference["log_fmax"][0]) < TIGHT and log_fmax[0, -1] < TOLERANCE
    # what a minimisation must leave alone, and the state forces() leaves
    assert torch.equal(md.v, v0) and torch.equal(md.log_pe, pe0) and torch.equal(md.log_ke, ke0) and int(md.counter.item()) == 0
    assert float(md.ene) == out[0]["energy"] and float(md.core.e_agbnp.abs().max()) == 0.0 and md.core.part_read == 0
    frc = md.frc.cpu().numpy()
    md.forces()
    assert k.finish() == 0
    assert np.abs(md.frc.cpu().numpy() - frc).max() < TIGHT
    energy_close(float(md.ene), out[0]["energy"])
    assert md.run(20, "verlet", check_every=20) == 0
    assert int(md.counter.item()) == 20


def test_replicas_minimise_as_device_md_runs(gpu_required, systems, five):
    """R = 3 from distinct perturbed starts against three DeviceMD.minimise runs alone from the same starts; the first replica
    to converge keeps its positions bit for bit at every later check (there is one after every iteration) while the others go on."""
    torch = pytest.importorskip("torch")
    from openmm_agbnp_plugin_amd.md import DeviceMD, ReplicaMD
    s = systems("trpcage")
    R = 3
    rep = ReplicaMD(s, [_kernel(s.params()) for _ in range(R)], [300.0] * R, seeds=[5, 6, 7], k_tether=K_TETHER)
    rep.settle()
    for r in range(R):
        rep.x[r].add_(0.002 * torch.sin(rep.x[r] * (37.0 + 3.0 * r)))
    starts, v0 = rep.x.clone(), rep.v.clone()
    assert float((starts[0] - starts[1]).abs().max()) > 1e-4  # (the replicas do not start as copies of one another)
    alone = []
    for r in range(R):
        k = _kernel(s.params())
        md = DeviceMD(s, k, k_tether=K_TETHER, seed=5 + r)
        md.settle()
        md.x.copy_(starts[r])
        out = md.minimise(tolerance=TOLERANCE, max_iterations=CAP)
        alone.append((out[0], md.x.cpu().numpy()))
    checks = []
    out = rep.minimise(tolerance=TOLERANCE, max_iterations=CAP, check_every=1, on_check=lambda c: checks.append((c.copy(), rep.x.cpu().numpy())))
    x = rep.x.cpu().numpy()
    oracle = _oracle(s)
    for r in range(R):
        _judge_final(f"replica {r}", s, oracle, x[r], out[r])
        de, dx = abs(out[r]["energy"] - alone[r][0]["energy"]), np.abs(x[r] - alone[r][1]).max()
        print(f"replica {r} against DeviceMD alone ({int(alone[r][0]['iterations'])} iterations): |dE| {de:.2e} kJ/mol  |dx| {dx:.2e} nm")
        assert de < 1e-3 and dx < 1e-3
    first = next(i for i, (c, _) in enumerate(checks) if c.any())
    for r in np.flatnonzero(checks[first][0]):
        for c, xc in checks[first:]:
            assert c[r] and np.array_equal(xc[r], checks[first][1][r]), f"converged replica {r} moved"
        assert np.array_equal(x[r], checks[first][1][r])
    print(f"iterations {out['iterations'].tolist()}; {len(checks) - 1 - first} checks behind the first convergence")
    assert torch.equal(rep.v, v0) and not rep.counter.any() and rep.core.part_read == 0
    assert list(rep.run(20, "verlet", check_every=20)) == [0] * R


def test_a_hamiltonian_ladder_relaxes_every_rung_under_its_own_parameters(gpu_required, systems, five):
    """R = 2, charges scaled by 1 and 0.95: each rung's force criterion holds under its own parameters (an oracle with those
    parameters), and an exchange() directly behind minimise() is judged as the host restatement judges it, from potentials that
    are the returned energies bit for bit."""
    pytest.importorskip("torch")
    from openmm_agbnp_plugin_amd.md import HamiltonianReplicaMD, hamiltonian_delta
    s = systems("trpcage")
    charges = [1.0 - 0.05 * k for k in range(2)]
    rep = HamiltonianReplicaMD(s, [_kernel(_scaled(s, q)) for q in charges], [300.0, 300.0], seeds=[61, 62], exchange_seed=5, k_tether=K_TETHER)
    rep.settle()
    out = rep.minimise(tolerance=TOLERANCE, max_iterations=CAP)
    x = rep.x.cpu().numpy()
    oracles = [_oracle(s, q) for q in charges]
    for k in range(2):
        _judge_final(f"rung {k} (charges x {charges[k]})", s, oracles[k], x[k], out[k])
    assert np.abs(x[0] - x[1]).max() > 1e-5 and abs(out[0]["energy"] - out[1]["energy"]) > 1.0  # (the rungs' minima differ)
    tether = rep.core.parts[0].cpu().numpy().sum(axis=1)
    rep.exchange()
    assert list(rep.finish()) == [0, 0]
    log = rep.exchange_log()
    assert len(log) == 1
    rec = log[0]
    assert rec["P_lo"] == out[0]["energy"] and rec["P_hi"] == out[1]["energy"]
    assert rec["T_lo"] == tether[0] and rec["T_hi"] == tether[1]
    energy_close(rec["C_lo"], float(oracles[0].execute(x[1])[0]))
    energy_close(rec["C_hi"], float(oracles[1].execute(x[0])[0]))
    delta = hamiltonian_delta(*(rec[key] for key in ("kT_lo", "kT_hi", "P_lo", "P_hi", "T_lo", "T_hi", "C_lo", "C_hi")))
    assert abs(np.log(rec["u"]) - delta) > 1e-12 * max(1.0, abs(delta))
    assert int(rec["accepted"]) == int(np.log(rec["u"]) <= delta)


def test_the_example_script_runs(gpu_required):
    """examples/minimise_agbnp.py on trpcage: it converges, reports nothing void or withheld, and equilibrates."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "minimise_agbnp.py"), "trpcage", "10.0", "200"],
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "minimised in " in out.stdout and "not converged" not in out.stdout and "void" not in out.stdout
    assert "Equilibration ..." in out.stdout and "\n200," in out.stdout and "WARNING" not in out.stdout
