"""The inputs of tests/test_gpu_boundaries.py and of tests/test_boundary_systems_oracle.py, which pins them on the CPU: atom pairs
placed ON a decision boundary of a pair kernel (`d2 < range2`, `d2 < gb_cut2`, the box culls beside them, the last interval of the
I4 table), exact ties in the sibling order of the overlap tree, and origins thousands of nm away.  A plain module like
tests/edge_systems.py: the test files import what they use.

Cutoff ties.  Positions snapped to the grid 1/128 nm: every coordinate difference is an integer / 128 and every squared distance an
integer m / 16384 -- exact in FP64 and in FP32 (m < 2^24) under any evaluation order, with or without FMA, and relative to any atom
of the system.  A cutoff c = sqrt(m) / 128 whose square IS m / 16384 in FP64 puts every pair at squared distance m exactly on
`d2 < cut2`; between sqrt(m - 0.5) / 128 and c the model is one (ties excluded), between nextafter(c, 2) and sqrt(m + 0.5) / 128 it is
another (ties included)."""
from fractions import Fraction

import numpy as np

import openmm_agbnp_plugin_amd as P
from openmm_agbnp_plugin_amd.systems import vdw_alpha_from_radius
from tests.edge_systems import size_edge

GRID = 128.0
GRID2 = GRID * GRID

# ---- 1. cutoff ties -----------------------------------------------------------------------------------------------------------
# m: of the m in TIE_WINDOW whose cutoff is exact (tie_cutoff), the one with the most tied pairs (pinned on the CPU)
TIE_M = {"1dwc": 16301, "trpcage": 11090}
TIE_WINDOW = (0.8, 1.0)  # nm: where the m above were looked for
TIE_COUNTS = {"1dwc": (184, 50, 92, 42), "trpcage": (9, 1, 5, 3)}  # tied pairs: all, heavy-heavy, heavy-H, H-H
# the CPU oracle (version 1) on the snapped systems: ties excluded (cutoff c), ties included (nextafter(c, 2))
TIE_ENERGY = {"1dwc": (-38300.26903399582, -38263.02666306114), "trpcage": (-2054.461201009006, -2071.233643051515)}


def snapped(s, name=None):
    """`s` with its positions on the grid."""
    return P.AGBNPSystem(name or f"{s.name}_snapped", np.rint(s.pos * GRID) / GRID, s.radius, s.gamma, s.alpha, s.charge, s.ishydrogen)


def grid_m(pos):
    """Squared distances of all pairs in units of 1 / 16384 nm^2, as exact integers [n, n]."""
    q = np.rint(pos * GRID).astype(np.int64)
    assert (q / GRID == pos).all(), "positions are not on the grid"
    d = q[:, None, :] - q[None, :, :]
    return (d * d).sum(axis=-1)


def tie_cutoff(m):
    """c = sqrt(m) / 128 if c * c is m / 16384 bit for bit (then `d2 < c * c` sees the tie as the oracle does), else None."""
    c = float(np.sqrt(float(m))) / GRID
    return c if c * c == m / GRID2 else None


def cutoff_below(m):
    """A cutoff strictly between the squared distances m - 1 and m: the model of c (ties excluded), not on any boundary."""
    return float(np.sqrt(m - 0.5)) / GRID


def cutoff_above(m):
    """... between m and m + 1: the model of nextafter(c, 2) (ties included)."""
    return float(np.sqrt(m + 0.5)) / GRID


def tied_pairs(s, m):
    """(i, j), i < j, of the pairs at squared distance exactly m / 16384."""
    i, j = np.nonzero(np.triu(grid_m(s.pos) == m, 1))
    return np.stack([i, j], axis=1)


def tie_counts(s, m):
    """(all, heavy-heavy, heavy-H, H-H)"""
    pairs = tied_pairs(s, m)
    nh = s.ishydrogen[pairs].sum(axis=1)
    return len(pairs), int((nh == 0).sum()), int((nh == 1).sum()), int((nh == 2).sum())


# ---- 2. a block box at the cutoff ---------------------------------------------------------------------------------------------
# (heavy atoms, atoms) of the size edges of 1dwc that make a copy: whole blocks, so that no block -- in atom order or in pair order
# (heavy atoms first) -- holds atoms of both copies.  (128, 256): two heavy, two hydrogen and four atom blocks per copy; the closest
# pair meets in a GB strip and a heavy x H tile.  (64, 64): one block per copy; the pair meets in the GB tile (0, 1) and the
# symmetric heavy x heavy tile (0, 1), whose culls are written separately from the strips'.
BOX_SIZES = ((128, 256), (64, 64))
BOX_GAP_STEPS = 120       # grid steps between the copies' boxes along x: 0.9375 nm, m = 14400


def box_pair_name(nh, n):
    return f"box_pair_{nh}_{n}"


def box_pair(nh, n):
    """-> system, m of the closest cross-copy pairs, their (i, j).  Two copies of the snapped size edge, the second moved along x
    by a pitch on the grid, and along y and z (on the grid too) so that its atom of least x lies exactly behind the first copy's
    atom of greatest x: that pair is separated along x alone, by the gap of the copies' boxes, which is also the gap of the two
    blocks that hold the pair.  Every other cross-copy pair is further apart.  The gap is BOX_GAP_STEPS grid steps, so m is a
    square and the cutoff c = BOX_GAP_STEPS / 128 is exact: at c the blocks' gap2 EQUALS cut2 (`>=` culls), at sqrt(m + 0.5) / 128
    it is 0.5 / 16384 = 3e-5 nm^2 below it and the one pair counts."""
    base = snapped(size_edge(P.load_system("1dwc"), nh, n))
    a, b = int(np.argmax(base.pos[:, 0])), int(np.argmin(base.pos[:, 0]))
    shift = base.pos[a] - base.pos[b] + np.array([BOX_GAP_STEPS / GRID, 0.0, 0.0])
    s = P.AGBNPSystem(box_pair_name(nh, n), np.concatenate([base.pos, base.pos + shift]), *[np.tile(v, 2) for v in base.params()])
    cross = grid_m(s.pos)[:n, n:]
    m = int(cross.min())
    i, j = np.nonzero(cross == m)
    return s, m, np.stack([i, j + n], axis=1)


def gb_item_kind(block_i, block_j):
    """How the GB tile launch meets two 64-atom blocks (atom order; allocate_work in csrc/engine_setup.hip): blocks 2p and 2p + 1
    with each other and with themselves in 64 x 64 tiles, with every later block in a strip."""
    return "tile" if block_i // 2 == block_j // 2 else "strip"


def block_gap2(pos, block_i, block_j):
    """Squared gap between the boxes of two sets of atoms, in nm^2 (box_gap2 / strip_gap2 of csrc/pair_bodies.h)."""
    lo_i, hi_i, lo_j, hi_j = pos[block_i].min(axis=0), pos[block_i].max(axis=0), pos[block_j].min(axis=0), pos[block_j].max(axis=0)
    return float((np.maximum(0.0, np.maximum(lo_j - hi_i, lo_i - hi_j)) ** 2).sum())


# ---- 3. the last interval of the I4 table -------------------------------------------------------------------------------------
PROBE_SUBSET = 40          # the first atoms of trpcage
PROBE_CENTRE_RADIUS = 0.21   # nm: the largest radius class of the system, so that A's screener type is the last of every slice
ULP4 = 2.0 ** -51          # the spacing of FP64 below 4


def fma(a, b, c):
    """fma(a, b, c) of FP64 in exact rational arithmetic, rounded once (to nearest even, as float(Fraction) rounds)."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def d2_as_the_kernels_form_it(d):
    return fma(d[2], d[2], fma(d[1], d[1], float(Fraction(d[0]) * Fraction(d[0]))))


def probe_offsets():
    """(name, offset from A, k, radius, ishydrogen): squared distance to A exactly 4 - k 2^-51 as the kernels form it (k = 0: exactly
    4.0, excluded).  One FP64 step under 2 along an axis gives k = 2; a second coordinate of 2^-25.5 beside it gives k = 1."""
    near = 2.0 - 2.0 ** -52
    tiny = float(np.sqrt(2.0 ** -51))
    return (
        ("heavy, k = 2, A's radius", np.array([near, 0.0, 0.0]), 2, PROBE_CENTRE_RADIUS, 0),
        ("hydrogen, k = 2", np.array([-near, 0.0, 0.0]), 2, 0.121, 1),
        ("heavy, k = 1, a common radius", np.array([tiny, near, 0.0]), 1, 0.17, 0),
        ("hydrogen, k = 1", np.array([tiny, -near, 0.0]), 1, 0.121, 1),
        ("heavy, d2 = 4", np.array([0.0, 0.0, 2.0]), 0, PROBE_CENTRE_RADIUS, 0),
    )


def probe_system():
    """-> system, index of A, indices of the probes (in the order of probe_offsets).  The first 40 atoms of trpcage, moved so that
    the heavy atom A nearest their centre is EXACTLY at the origin (a difference to A is then the other atom's coordinate, bit for
    bit, in either order of subtraction up to its sign), A's radius raised to PROBE_CENTRE_RADIUS, and the probes appended."""
    base = P.load_system("trpcage").subset(np.arange(PROBE_SUBSET))
    heavy = np.flatnonzero(base.ishydrogen == 0)
    a = int(heavy[np.argmin(np.linalg.norm(base.pos[heavy] - base.pos.mean(axis=0), axis=1))])
    pos = base.pos - base.pos[a]
    assert (pos[a] == 0.0).all()
    offsets = probe_offsets()
    radius = np.concatenate([base.radius, [o[3] for o in offsets]])
    radius[a] = PROBE_CENTRE_RADIUS
    ish = np.concatenate([base.ishydrogen, np.array([o[4] for o in offsets], dtype=np.int32)])
    gamma = np.concatenate([base.gamma, [0.0 if o[4] else base.gamma[a] for o in offsets]])  # (one gamma for all heavy atoms)
    charge = np.concatenate([base.charge, [0.25, -0.25, 0.2, -0.2, 0.1]])
    s = P.AGBNPSystem("i4_probes", np.concatenate([pos, np.stack([o[1] for o in offsets])]), radius, gamma, vdw_alpha_from_radius(radius),
                      charge, ish)
    return s, a, list(range(base.n, base.n + len(offsets)))


# ---- 4. exact ties in the sibling order of the tree ---------------------------------------------------------------------------
LATTICE_SIDES = (4, 5)
LATTICE_SPACING = 0.25  # nm


def tie_lattice(side):
    """side^3 identical heavy atoms on a noise-free cubic lattice: every atom's neighbours of a shell have the same overlap volume."""
    n = side ** 3
    pos = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3) * LATTICE_SPACING
    radius = np.full(n, 0.19)
    charge = np.random.default_rng(100 + side).normal(0.0, 0.4, n)
    return P.AGBNPSystem(f"tie_lattice_{side}", pos, radius, np.full(n, 0.117 * 418.4), vdw_alpha_from_radius(radius), charge,
                         np.zeros(n, dtype=np.int32))


def lattice_permutation(side, k=0):
    return np.random.default_rng(1000 * side + k).permutation(side ** 3)


# ---- 5. far origins -----------------------------------------------------------------------------------------------------------
FAR_ORIGIN = np.array([512.0, -1024.0, 2048.0])  # nm: exact on the grid (a snapped coordinate of a few nm keeps its 7 fraction bits)


_table = {}


def boundary_systems():
    """name -> AGBNPSystem, built once: the snapped proteins, the box pair, the probes, the lattices."""
    if not _table:
        for name in TIE_M:
            _table[f"{name}_snapped"] = snapped(P.load_system(name))
        for nh, n in BOX_SIZES:
            _table[box_pair_name(nh, n)] = box_pair(nh, n)[0]
        _table["i4_probes"] = probe_system()[0]
        for side in LATTICE_SIDES:
            _table[f"tie_lattice_{side}"] = tie_lattice(side)
    return _table
