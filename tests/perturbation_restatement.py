"""The references of the perturbation-energy tests (tests/test_perturbation_restatement.py on the CPU,
tests/test_gpu_perturbation.py and tests/test_gpu_perturbation_group.py on the device).

`oracle_energy` is THE reference for one parameter set m: the energy Oracle(radius, gamma^m, alpha^m, charge^m, ish).execute()
returns at the positions -- what a context created with that set would compute.  (The oracle's constructor refuses heavy-atom
gammas that differ from one another and its update() does not: a set with per-atom gammas is built with a uniform gamma and
updated.)

`restate` is the formula the perturbation launch evaluates (include/agbnp_hip.h, agbnp_hip_perturbed_energies_*), from the
vectors of ONE base oracle -- the self volumes with both sets of radii and the Born radii depend on geometry and radii alone:

    E_m = sum_h (gamma_h^m / roffset) (sv_large_h - sv_vdw_h)        heavy atoms h; a hydrogen's gamma counts as 0
        + sum_i alpha_i^m / (B_i + 0.14 nm)^3
        + k sum_i (q_i^m)^2 / B_i  +  k sum_i q_i^m sum_{j != i} q_j^m f_ij

with f_ij of tests/decomposition_restatement.py (pair_sums: d^2 < cutoff^2 with a cutoff).  Version 0 has the first line only.
A plain module like tests/gpu_helpers.py: the test files import what they use."""
import numpy as np

from oracle import Oracle
from tests.decomposition_restatement import DIEL, HB_RADIUS, ROFFSET, pair_sums


def oracle_energy(radius, gamma, alpha, charge, ish, pos, version=1, cutoff=None, method=1):
    """The energy of a system created with these parameters, at pos."""
    gamma = np.asarray(gamma, dtype=np.float64)
    heavy = np.asarray(ish) == 0
    if heavy.any() and np.ptp(gamma[heavy]) != 0.0:
        uniform = np.where(heavy, gamma[heavy][0], 0.0)
        o = Oracle(radius, uniform, alpha, charge, ish, version=version, cutoff=cutoff, method=method)
        o.update(radius, gamma, alpha, charge, ish)
    else:
        o = Oracle(radius, gamma, alpha, charge, ish, version=version, cutoff=cutoff, method=method)
    return o.execute(np.asarray(pos, dtype=np.float64).reshape(-1, 3))[0]


def oracle_energies(params, sets, pos, version=1, cutoff=None, method=1):
    """oracle_energy for every (gamma, alpha, charge) of `sets`, with the radii and hydrogen flags of `params`."""
    radius, ish = params[0], params[4]
    return np.array([oracle_energy(radius, g, a, q, ish, pos, version, cutoff, method) for g, a, q in sets])


def restate(params, sets, pos, version=1, cutoff=None, method=1):
    """(the base oracle's own energy, E[M]) from one Oracle.execute() with the parameters `params`."""
    radius, _, _, _, ish = [np.asarray(p) for p in params]
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    if method == 0:
        cutoff = None
    o = Oracle(*params, version=version, cutoff=cutoff, method=method)
    own, _ = o.execute(pos)
    area = np.where(ish != 0, 0.0, o.vector("selfvol_large") - o.vector("selfvol_vdw")) / ROFFSET
    out = np.zeros(len(sets))
    born = o.vector("born") if version == 1 else None
    for m, (gamma, alpha, charge) in enumerate(sets):
        out[m] = (np.asarray(gamma, dtype=np.float64) * area).sum()
        if version != 1:
            continue
        q = np.asarray(charge, dtype=np.float64)
        out[m] += (np.asarray(alpha, dtype=np.float64) / (born + HB_RADIUS) ** 3).sum()
        out[m] += DIEL * ((q * q / born).sum() + (q * pair_sums(pos, q, born, cutoff)).sum())
    return own, out


def standard_sets(params, seed=7):
    """The four sets of the CPU test: the charges scaled (with alpha), gamma scaled, a per-atom gamma, every charge zero."""
    _, gamma, alpha, charge, ish = [np.asarray(p, dtype=np.float64) for p in params]
    rng = np.random.default_rng(seed)
    per_atom = np.where(ish != 0, 0.0, gamma * rng.uniform(0.5, 1.5, len(gamma)))
    return [(gamma, 1.1 * alpha, 0.9 * charge), (0.5 * gamma, alpha, charge), (per_atom, alpha, charge),
            (gamma, alpha, np.zeros_like(charge))]


def ladder(params, count):
    """`count` distinct sets: a charge-scaling ladder q (1 - 0.05 m) with gamma (1 - 0.02 m) and alpha (1 + 0.03 m); rung 0 is
    the system's own parameters."""
    _, gamma, alpha, charge, _ = [np.asarray(p, dtype=np.float64) for p in params]
    return [((1.0 - 0.02 * m) * gamma, (1.0 + 0.03 * m) * alpha, (1.0 - 0.05 * m) * charge) for m in range(count)]


def tables(sets):
    """The sets as the three [M, N] arrays set_parameter_sets() takes."""
    return tuple(np.array([s[k] for s in sets], dtype=np.float64) for k in range(3))
