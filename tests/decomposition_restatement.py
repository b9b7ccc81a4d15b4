"""The reference of every per-atom decomposition test (tests/test_decomposition_restatement.py on the CPU,
tests/test_gpu_decomposition.py on the device): a NumPy restatement of the four per-atom terms of include/agbnp_hip.h
(agbnp_hip_decompose_*), built from the CPU oracle's own vectors -- the self volumes with the enlarged and the vdW radii and the
Born radii of one Oracle.execute() -- and the formulas

    plane 0  cavity    nu_i (sv_large_i - sv_vdw_i),  nu_i = gamma_i / roffset (0 for a hydrogen)
    plane 1  vdW       alpha_i / (B_i + 0.14 nm)^3
    plane 2  GB self   k q_i^2 / B_i
    plane 3  GB pair   k q_i sum_{j != i} q_j / sqrt(d^2 + B_i B_j exp(-d^2 / (4 B_i B_j)))     (d^2 < cutoff^2 with a cutoff)

with the constants as the reference writes them (roffset = 0.5f * 0.1f and 1.4 * 0.1f promoted to double).  Version 0 has plane 0
only.  A plain module like tests/gpu_helpers.py: the test files import what they use."""
import numpy as np

from oracle import Oracle

TERMS = ("cavity", "vdw", "gb_self", "gb_pair")
ROFFSET = float(np.float32(0.5) * np.float32(0.1))
HB_RADIUS = 1.4 * float(np.float32(0.1))
DIEL = (4.184 * 332.0 / 10.0) * (-0.5) * (1.0 / 1.0 - 1.0 / 80.0)
CHUNK = 256  # rows of a pair block: 1dwc needs no N x N x 3 array


def pair_sums(pos, charge, born, cutoff=None):
    """sum_{j != i} q_j f_ij for every atom i, in row chunks."""
    n = len(charge)
    out = np.zeros(n)
    for lo in range(0, n, CHUNK):
        hi = min(n, lo + CHUNK)
        d2 = ((pos[lo:hi, None, :] - pos[None, :, :]) ** 2).sum(axis=-1)
        bb = born[lo:hi, None] * born[None, :]
        f = 1.0 / np.sqrt(d2 + bb * np.exp(-0.25 * d2 / bb))
        f[np.arange(hi - lo), np.arange(lo, hi)] = 0.0
        if cutoff is not None:
            f[d2 >= cutoff * cutoff] = 0.0
        out[lo:hi] = f @ charge
    return out


def restate(params, pos, version=1, cutoff=None, method=1):
    """(energy of Oracle.execute, terms[4, N], the oracle) at `pos`.  cutoff: the fast mode's (Oracle(cutoff=...)); method 0
    (NoCutoff) drops it, as the oracle does."""
    radius, gamma, alpha, charge, ish = [np.asarray(p) for p in params]
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    if method == 0:
        cutoff = None
    o = Oracle(*params, version=version, cutoff=cutoff, method=method)
    energy, _ = o.execute(pos)
    n = len(radius)
    terms = np.zeros((len(TERMS), n))
    nu = np.where(ish != 0, 0.0, np.asarray(gamma, dtype=np.float64) / ROFFSET)
    terms[0] = nu * (o.vector("selfvol_large") - o.vector("selfvol_vdw"))
    if version == 1:
        born = o.vector("born")
        q = np.asarray(charge, dtype=np.float64)
        terms[1] = np.asarray(alpha, dtype=np.float64) / (born + HB_RADIUS) ** 3
        terms[2] = DIEL * q * q / born
        terms[3] = DIEL * q * pair_sums(pos, q, born, cutoff)
    return energy, terms, o


def surface_areas(terms, gamma):
    """The GaussVol surface area of every atom, A_i = cavity term / gamma_i (0 where gamma is 0)."""
    gamma = np.asarray(gamma, dtype=np.float64)
    return np.divide(terms[0], gamma, out=np.zeros_like(gamma), where=gamma != 0.0)
