"""The inputs of tests/test_gpu_edge_regimes.py and of tests/test_edge_systems_oracle.py, which pins them on the CPU: a table
name -> AGBNPSystem of sizes at the edges of the engine's blocks (64 heavy atoms, 256 atoms, the 32-atom padding of an OpenMM
context, no heavy atom at all, a single atom) and of a cluster whose Born radii reach the 2 nm cap of the reference's
ReferenceAGBNPKernels.cpp:41-55 (beta < 0: 1/B = 1/2 nm, f' = 0), which no other input of the suite does.  A plain module like
tests/gpu_helpers.py: the test files import what they use."""
import numpy as np

import openmm_agbnp_plugin_amd as P
from openmm_agbnp_plugin_amd.systems import vdw_alpha_from_radius

# (heavy atoms, atoms): the first nh heavy atoms and the first n - nh hydrogens of 1dwc, in the file's order
SIZE_EDGES = ((0, 1), (1, 1), (0, 32), (1, 33), (64, 64), (65, 65), (64, 128), (64, 256), (63, 255), (127, 255), (128, 256), (129, 257),
              (256, 512), (257, 513))
FAR_PITCHES = (24.0, 27.0)  # nm, either side of sqrt(4 * 60 ln2 * 2 * 2) = 25.8 nm: the far-strip bound of two blocks of capped Born radii

# what the CPU oracle gives for the born_clamp family (version 1; pinned by tests/test_edge_systems_oracle.py)
ORACLE_ENERGY = {
    "born_clamp": -666.738148959264,
    "born_clamp_q0": 57.18419016968724,
    "born_clamp_pair_24": -1384.9435777972526,
    "born_clamp_pair_27": -1379.2250037376496,
}


def size_edge_name(nh, n):
    return f"size_{nh}_{n}"


def size_edge(base, nh, n):
    """`base` is 1dwc."""
    heavy = np.flatnonzero(base.ishydrogen == 0)[:nh]
    hydrogens = np.flatnonzero(base.ishydrogen == 1)[: n - nh]
    assert len(heavy) == nh and len(hydrogens) == n - nh
    s = base.subset(sorted(list(heavy) + list(hydrogens)))
    s.name = size_edge_name(nh, n)
    return s


def born_clamp():
    """21 atoms: eight heavy atoms of radius 0.30 nm around a heavy atom of radius 0.15 nm and twelve hydrogens, all within a few
    tenths of a nm: the descreening sums of the inner atoms exceed 1/R, so beta < 0 and their Born radii sit at the 2 nm cap."""
    rng = np.random.default_rng(8)
    pos = np.concatenate([rng.normal(0, 0.15, (8, 3)), rng.normal(0, 0.075, (1, 3)), rng.normal(0, 0.075, (12, 3))])
    radius = np.concatenate([np.full(8, 0.30), np.full(1, 0.15), np.full(12, 0.121)])
    ish = np.concatenate([np.zeros(9, dtype=np.int32), np.ones(12, dtype=np.int32)])
    gamma = np.where(ish == 1, 0.0, 0.117 * 418.4)
    charge = rng.normal(0, 0.4, 21)
    return P.AGBNPSystem("born_clamp", pos, radius, gamma, vdw_alpha_from_radius(radius), charge, ish)


def born_clamp_family():
    s = born_clamp()
    out = {"born_clamp": s}
    out["born_clamp_q0"] = P.AGBNPSystem("born_clamp_q0", s.pos, s.radius, s.gamma, s.alpha, np.zeros(s.n), s.ishydrogen)
    for pitch in FAR_PITCHES:
        pair = P.lattice(s, 2, 1, 1, pitch)
        pair.name = f"born_clamp_pair_{pitch:.0f}"
        out[pair.name] = pair
    return out


def born_clamp_strip(gap):
    """The pairs above are 42 atoms: ONE 64-atom block, a diagonal tile, no strip.  The GB stage's strips (gb_strip in
    csrc/pair_bodies.h) meet blocks 2p and 2p + 1 with a block J >= 2p + 2, so the far-strip test needs three blocks: here blocks
    0 and 1 are six copies of born_clamp in a row along y (3 nm apart: beyond the tables' 2 nm reach, every copy keeps its eleven
    capped atoms) and two lone hydrogens, 128 atoms; block 2 is a seventh copy whose box lies `gap` nm beyond theirs along x."""
    s = born_clamp()
    extent = s.pos[:, 0].max() - s.pos[:, 0].min()
    assert s.pos[:, 0].min() < 0.0 < s.pos[:, 0].max()
    offsets = [np.array([0.0, 3.0 * k, 0.0]) for k in range(6)]
    lone = np.array([[0.0, 18.0, 0.0], [0.0, 18.5, 0.0]])
    pos = np.concatenate([s.pos + o for o in offsets] + [lone, s.pos + np.array([extent + gap, 0.0, 0.0])])

    def tiled(a, lone_values):
        return np.concatenate([np.tile(a, 6), np.asarray(lone_values, dtype=a.dtype), a])

    radius = tiled(s.radius, [0.121, 0.121])
    return P.AGBNPSystem(f"born_clamp_strip_{gap:.0f}", pos, radius, tiled(s.gamma, [0.0, 0.0]), vdw_alpha_from_radius(radius),
                         tiled(s.charge, [0.3, -0.3]), tiled(s.ishydrogen, [1, 1]))


def block_gap(s, pos=None):
    """The gap between the boxes of atom blocks {0, 1} and 2 as the far-strip test measures it (strip_gap2 in csrc/pair_bodies.h)."""
    pos = s.pos if pos is None else pos
    lo, hi = [pos[64 * b: 64 * b + 64].min(axis=0) for b in range(3)], [pos[64 * b: 64 * b + 64].max(axis=0) for b in range(3)]
    return min(float(np.sqrt((np.maximum(0.0, np.maximum(lo[2] - hi[b], lo[b] - hi[2])) ** 2).sum())) for b in (0, 1))


# 12 nm: far below the bound of capped radii, yet beyond the bound of any Born radius under 0.93 nm (every other input of the suite):
# a strip taken for far there is wrong in the sixth digit of the energy.  24 and 27 nm: either side of the bound, as the pairs are
STRIP_GAPS = (12.0,) + FAR_PITCHES
STRIP_NAMES = tuple(f"born_clamp_strip_{gap:.0f}" for gap in STRIP_GAPS)
NAMES = tuple(size_edge_name(nh, n) for nh, n in SIZE_EDGES) + tuple(ORACLE_ENERGY) + STRIP_NAMES

_table = {}


def edge_systems():
    """The whole table, built once."""
    if not _table:
        base = P.load_system("1dwc")
        for nh, n in SIZE_EDGES:
            _table[size_edge_name(nh, n)] = size_edge(base, nh, n)
        _table.update(born_clamp_family())
        for gap in STRIP_GAPS:
            strip = born_clamp_strip(gap)
            _table[strip.name] = strip
        assert tuple(_table) == NAMES
    return _table
