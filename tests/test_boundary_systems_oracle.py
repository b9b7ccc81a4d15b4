"""CPU: pins the inputs of tests/test_gpu_boundaries.py (tests/boundary_systems.py) with the oracle, so that the GPU tests cannot
silently stop standing on their boundaries: the tied pairs ARE at the cutoff bit for bit and number what the table says, the
oracle has exactly two models around each tie and they differ by far more than any tolerance, the box pair's blocks ARE a cutoff
apart, the probes' squared distances are 4 - k 2^-51 bit for bit and index the table entries they are meant to, the noise-free
lattices do not depend on the order of their atoms, and the far translation is exact."""
import numpy as np
import pytest

import openmm_agbnp_plugin_amd as P
from oracle import Oracle
from tests import boundary_systems as B

TIE_NAMES = tuple(B.TIE_M)


@pytest.fixture(scope="module")
def table():
    return B.boundary_systems()


@pytest.mark.parametrize("name", TIE_NAMES)
def test_the_tie_cutoff_is_exact_and_has_the_most_ties_of_its_window(table, name):
    s = table[f"{name}_snapped"]
    m = B.TIE_M[name]
    c = B.tie_cutoff(m)
    assert c is not None and c * c == m / B.GRID2
    assert np.float32(c * c) == np.float32(m / B.GRID2)  # (the float cutoff of the single-precision forms is the tie too)
    assert abs(c - {"1dwc": 0.997463824923616, "trpcage": 0.822727101056298}[name]) < 1e-15
    assert B.tie_counts(s, m) == B.TIE_COUNTS[name]
    ms = B.grid_m(s.pos)[np.triu_indices(s.n, 1)]
    lo, hi = B.TIE_WINDOW
    values, counts = np.unique(ms[(ms >= lo * lo * B.GRID2) & (ms <= hi * hi * B.GRID2)], return_counts=True)
    exact = np.array([B.tie_cutoff(int(v)) is not None for v in values])
    assert 0.4 < exact.mean() < 0.7  # (about half of all m have an exact cutoff)
    assert counts[exact].max() == B.TIE_COUNTS[name][0] and int(values[exact][np.argmax(counts[exact])]) == m
    assert ms.max() < 2 ** 24  # every squared distance is exact in FP32 as well


def test_ties_of_1dwc_cross_the_engines_blocks(table):
    """The engine blocks its atoms by 64 in two orders (csrc/engine_setup.hip): atom order -- the file's -- for the GB tiles and
    strips, and pair order -- heavy atoms in the file's order, then hydrogens, each padded to whole blocks -- for the Born and
    chain-rule tiles.  Both are obtainable on the host.  (The row form has no blocks: a row is one atom and its list.)"""
    s = table["1dwc_snapped"]
    pairs = B.tied_pairs(s, B.TIE_M["1dwc"])
    assert int((pairs[:, 0] // 64 != pairs[:, 1] // 64).sum()) >= 100
    kinds = [B.gb_item_kind(i // 64, j // 64) for i, j in pairs]  # with AGBNP_HIP_ROWS=0 one GB launch holds tiles AND strips
    assert (kinds.count("tile"), kinds.count("strip")) == (26, 158)
    assert int((pairs[:, 0] // 64 == pairs[:, 1] // 64).sum()) == 12 and int((pairs[:, 0] // 128 == pairs[:, 1] // 128).sum()) == 26
    rank = np.where(s.ishydrogen == 0, np.cumsum(s.ishydrogen == 0) - 1, (s.nheavy + 63) // 64 * 64 + np.cumsum(s.ishydrogen == 1) - 1)
    born = pairs[s.ishydrogen[pairs].sum(axis=1) < 2]  # (two hydrogens do not descreen each other)
    assert int((rank[born[:, 0]] // 64 != rank[born[:, 1]] // 64).sum()) >= 100
    assert int((rank[born[:, 0]] // 64 == rank[born[:, 1]] // 64).sum()) >= 1  # (and a diagonal tile holds one)


@pytest.mark.parametrize("name", TIE_NAMES)
def test_the_oracle_has_two_models_around_the_tie(table, name):
    """E and F at c, nextafter(c, 0) and sqrt(m - 0.5) / 128 are one result bit for bit (the oracle excludes a tie: `>= cutoff2`);
    at nextafter(c, 2) and sqrt(m + 0.5) / 128 another; the two energies are the recorded ones and more than 1 kJ/mol apart."""
    s = table[f"{name}_snapped"]
    m = B.TIE_M[name]
    c = B.tie_cutoff(m)
    run = lambda cutoff: Oracle(*s.params(), version=1, cutoff=cutoff).execute(s.pos)  # noqa: E731
    e_out, f_out = run(c)
    e_in, f_in = run(float(np.nextafter(c, 2.0)))
    for cutoff in (float(np.nextafter(c, 0.0)), B.cutoff_below(m)):
        e, f = run(cutoff)
        assert e == e_out and (f == f_out).all()
    e, f = run(B.cutoff_above(m))
    assert e == e_in and (f == f_in).all()
    assert abs(e_out - B.TIE_ENERGY[name][0]) < 1e-9 and abs(e_in - B.TIE_ENERGY[name][1]) < 1e-9
    assert abs(e_in - e_out) > 1.0
    jump, df = {"1dwc": (37.24, 41.0), "trpcage": (16.77, 9.1)}[name]
    assert abs(abs(e_in - e_out) - jump) < 0.01 and abs(np.abs(f_in - f_out).max() / df - 1.0) < 0.05


@pytest.mark.parametrize("nh,n1", B.BOX_SIZES)
def test_the_box_pair_puts_two_blocks_a_cutoff_apart(table, nh, n1):
    s = table[B.box_pair_name(nh, n1)]
    again, m, pairs = B.box_pair(nh, n1)
    n = s.n // 2
    assert (again.pos == s.pos).all() and (s.nheavy, s.n) == (2 * nh, 2 * n1)
    assert m == B.BOX_GAP_STEPS ** 2 and B.tie_cutoff(m) == B.BOX_GAP_STEPS / B.GRID
    assert len(pairs) == 1  # k: the cross-copy pairs inside sqrt(m + 0.5) / 128; none is inside c
    cross = B.grid_m(s.pos)[:n, n:]
    assert int((cross < m).sum()) == 0 and int((cross < m + 0.5).sum()) == 1 and int((cross <= m + 1).sum()) == 1
    i, j = (int(v) for v in pairs[0])
    # (128, 256): a heavy atom and a hydrogen; (64, 64): two heavy atoms -- either pair is in the Born, GB and chain-rule stages
    assert sorted(s.ishydrogen[[i, j]]) == ([0, 1] if n1 > nh else [0, 0])
    # atom order (GB tiles and strips): the two blocks' gap2 IS cut2 at c, and 0.5 / 16384 nm^2 under it at the upper cutoff
    block = lambda a: np.arange(a // 64 * 64, a // 64 * 64 + 64)  # noqa: E731
    assert i // 64 < n // 64 <= j // 64
    assert B.gb_item_kind(i // 64, j // 64) == ("strip" if n1 == 256 else "tile")
    gap2 = B.block_gap2(s.pos, block(i), block(j))
    assert gap2 == m / B.GRID2 == B.tie_cutoff(m) ** 2
    assert 0.0 < B.cutoff_above(m) ** 2 - gap2 < 1e-4
    if n1 == 256:  # a strip meets blocks 2p and 2p + 1 with one block J: the partner of i's block is no nearer
        assert B.block_gap2(s.pos, block((i // 64 ^ 1) * 64), block(j)) >= gap2
    # pair order (Born and chain-rule tiles): the heavy blocks, then the hydrogen blocks, are the copies' in turn
    heavy, hydrogens = np.flatnonzero(s.ishydrogen == 0), np.flatnonzero(s.ishydrogen == 1)
    of = lambda ids, atom: ids[int(np.searchsorted(ids, atom)) // 64 * 64:][:64]  # noqa: E731
    bi, bj = (of(hydrogens if s.ishydrogen[a] else heavy, a) for a in (i, j))
    assert len(bi) == len(bj) == 64 and (bi < n).all() and (bj >= n).all()
    assert B.block_gap2(s.pos, bi, bj) == m / B.GRID2
    # no other pair of cross-copy blocks is nearer than these, in either order
    for ids in (np.arange(s.n), np.concatenate([heavy, hydrogens])):
        blocks = ids.reshape(-1, 64)
        first = [b for b in blocks if (b < n).all()]
        second = [b for b in blocks if (b >= n).all()]
        assert len(first) == len(second) == n1 // 64
        assert min(B.block_gap2(s.pos, p, q) for p in first for q in second) == m / B.GRID2


@pytest.mark.parametrize("nh,n1", B.BOX_SIZES)
def test_the_box_pairs_oracle_sees_the_one_pair(table, nh, n1):
    s = table[B.box_pair_name(nh, n1)]
    m = B.BOX_GAP_STEPS ** 2
    e_out, _ = Oracle(*s.params(), version=1, cutoff=B.tie_cutoff(m)).execute(s.pos)
    e_in, _ = Oracle(*s.params(), version=1, cutoff=B.cutoff_above(m)).execute(s.pos)
    assert abs(e_in - e_out) > 1e-3  # (7 and 58 kJ/mol: the charges of the pair are 0.06, -0.8 and -0.5, -0.8)
    base = B.snapped(B.size_edge(P.load_system("1dwc"), nh, n1))
    e_one, _ = Oracle(*base.params(), version=1, cutoff=B.tie_cutoff(m)).execute(base.pos)
    assert abs(e_out - 2.0 * e_one) < 1e-9 * abs(e_out)  # at c the copies do not see each other at all


def test_the_probes_stand_on_the_last_steps_under_four(table):
    s, a, probes = B.probe_system()
    assert (table["i4_probes"].pos == s.pos).all()
    assert (s.pos[a] == 0.0).all() and s.ishydrogen[a] == 0
    seen = []
    for (what, offset, k, radius, ish), p in zip(B.probe_offsets(), probes):
        for d in (s.pos[p] - s.pos[a], s.pos[a] - s.pos[p]):  # either order of subtraction
            assert (np.abs(d) == np.abs(offset)).all()
            d2 = B.d2_as_the_kernels_form_it(d)
            assert d2 == 4.0 - k * B.ULP4, what  # bit for bit
        assert (d2 < 4.0) == (k > 0)
        assert float(np.float32(d2)) == 4.0  # single precision cannot tell: there the pair is out (`d2 < 4.0f`)
        assert (s.radius[p], s.ishydrogen[p]) == (radius, ish)
        seen.append((k, ish))
    assert sorted(seen) == [(0, 0), (1, 0), (1, 1), (2, 0), (2, 1)]
    others = np.delete(np.arange(s.n), [a] + probes)
    for p in probes:  # a probe overlaps nobody (its other pairs are ordinary ones), and no probe is within the tables' reach of another
        assert np.linalg.norm(s.pos[others] - s.pos[p], axis=1).min() > 1.0
        assert all(np.linalg.norm(s.pos[q] - s.pos[p]) > 2.2 for q in probes if q != p)


def test_the_probed_type_pairs_are_the_last_of_a_slice_and_not(table):
    """The FP64 rows index entry (screened type * ntj + screener type) * 15 + (int)u of a table without padding: u = 15 from the last
    screener type reads the next screened type's first interval; from the last entry of all it reads past the table."""
    s, a, probes = B.probe_system()
    t = P.host_tables(s.radius, s.ishydrogen)
    nti, ntj = t["y"].shape[:2]
    screened, screener = t["type_screened"], t["type_screener"]
    assert (screened[a], screener[a]) == (nti - 1, ntj - 1)
    heavy2, hydrogen2, heavy1, hydrogen1, heavy0 = probes
    assert (screened[heavy2], screener[heavy2]) == (nti - 1, ntj - 1)        # A and this probe, both ways: the table's last entry
    assert screened[hydrogen2] == screened[hydrogen1] == 0                   # A descreens a hydrogen: the last entry of slice 0
    assert 0 < screened[heavy1] < nti - 1 and 0 < screener[heavy1] < ntj - 1  # A descreens it: the last of a middle slice; it descreens A: no last entry
    assert np.abs(t["y"][:, :, -1]).max() < 1e-12                            # the tables end in zero ...
    # ... and a read of the next slice's first interval shows where that slice is a small atom's: for the hydrogen probes it is
    # Q(0) = 15.6 / nm of the next hydrogen class under the smallest heavy atom, eight orders above TIGHT in a descreening sum.  (Under
    # the middle slice of the heavy probe lies A's own: Q(0) = 0 of a large atom screened by a small one.  That probe stands for
    # the pair that is NOT the last of its slice in the other direction.)
    assert t["y"][1, 0, 0] > 15.0 and abs(t["y"][nti - 1, 0, 0]) < 1e-12
    e, f = Oracle(*s.params(), version=1).execute(s.pos)
    assert np.isfinite(e) and np.isfinite(f).all()


@pytest.mark.parametrize("version", [0, 1])
@pytest.mark.parametrize("side", B.LATTICE_SIDES)
def test_the_noise_free_lattices_do_not_depend_on_the_order_of_their_atoms(table, side, version):
    s = table[f"tie_lattice_{side}"]
    assert s.n == side ** 3 and s.nheavy == s.n
    o = Oracle(*s.params(), version=version)
    e, f = o.execute(s.pos)
    stats = o.tree_stats()
    assert stats["max_subtree"] <= 777 and stats["level_counts"][7] == 0
    for k in range(3):
        perm = B.lattice_permutation(side, k)
        assert (perm != np.arange(s.n)).any()
        sp = s.permuted(perm)
        ep, fp = Oracle(*sp.params(), version=version).execute(sp.pos)
        assert abs(ep - e) < 1e-9 and np.abs(fp - f[perm]).max() < 1e-9


def test_the_far_translation_is_exact(table):
    s = table["trpcage_snapped"]
    far = s.pos + B.FAR_ORIGIN
    assert ((far - B.FAR_ORIGIN) == s.pos).all()
    assert (B.grid_m(far) == B.grid_m(s.pos)).all()
    assert np.abs(far).min() > 500.0
    # (a float still holds the grid at 2048 nm -- steps of 2^-12 nm against 2^-7 -- but nothing finer: a position off the grid is
    # lost to 1e-4 nm there, which is why the single-precision forms subtract a row's or block's first atom in FP64 first)
    assert (far.astype(np.float32).astype(np.float64) == far).all()
    assert float(np.float32(2048.0 + 1e-5)) == 2048.0
    e, f = Oracle(*s.params(), version=1).execute(s.pos)
    ef, ff = Oracle(*s.params(), version=1).execute(far)
    assert abs(ef - e) < 1e-9 and np.abs(ff - f).max() < 1e-9
