"""GPU box: atom pairs ON the decision boundaries of the pair kernels (tests/boundary_systems.py; pinned on the CPU by
tests/test_boundary_systems_oracle.py).  Every other input of the suite is generic geometry: a `<=` for a `<` in one of the forms
that write `d2 < range2` / `d2 < gb_cut2` out separately, a block box a little too small, or a float cutoff rounded the wrong way
would pass it.

1. Exact cutoff ties in fast mode: positions on the grid 1/128 nm, a cutoff whose square is a squared distance bit for bit.
2. A block box exactly at the cutoff: the workgroup-uniform culls `box_gap2 >= range2`, `strip_gap2 >= gb_cut2`.
3. The last interval of the I4 table: squared distances one and two steps of FP64 under 4 nm^2, and exactly 4.
4. Exact ties in the sibling order of the tree: noise-free lattices, in the file's order and permuted.
5. Origins thousands of nm away.

The forms: the default row form; AGBNP_HIP_ROWS=0, whose GB launch holds the 64 x 64 tiles (blocks 2p, 2p + 1 and the diagonal) AND
the strips (every other pair of blocks) at once -- no setting runs GB as tiles alone, and the ties of 1dwc lie in both (26 and 158);
fast+single.  A fresh context per cutoff and form, evaluated twice: the second evaluation runs packed forests and existing lists.

The reference is the CPU oracle, computed once per module for each (system, version, cutoff, geometry); the tolerances are those of
tests/gpu_helpers.py, FAST_TOL of tests/test_gpu_parity.py, and for fast+single the bounds of
test_fast_single_mode_rows_against_the_cutoff_oracle.  Every comparison prints |dE| and max|dF| first."""
import numpy as np
import pytest

import openmm_agbnp_plugin_amd as P
from oracle import Oracle
from tests import boundary_systems as B
from tests.gpu_helpers import SAME, TIGHT, Buffers, close, kernel_of
from tests.openmm_context import OpenMMContext
from tests.test_gpu_parity import FAST_TOL

pytestmark = pytest.mark.gpu

FORMS = ("rows", "tiles")  # the row form; the tile kernels everywhere (GB: tiles and strips)

_oracle_results = {}


def _oracle(name, version=1, cutoff=None, geometry="file", pos=None):
    """(E, F) of the oracle, once per module; `geometry` names `pos` where it is not the system's own."""
    key = (name, version, cutoff, geometry)
    if key not in _oracle_results:
        s = B.boundary_systems()[name]
        e, f = Oracle(*s.params(), version=version, cutoff=cutoff).execute(s.pos if pos is None else pos)
        f.setflags(write=False)
        _oracle_results[key] = (e, f)
    return _oracle_results[key]


def _kernel(s, cutoff, mode, version=1):
    force = P.AGBNPForce.from_arrays(*s.params(), version=version)
    if cutoff is not None:
        force.setNonbondedMethod(P.AGBNPForce.CutoffNonPeriodic)
        force.setCutoffDistance(cutoff)
    k = P.HipCalcAGBNPForceKernel(mode=mode)
    k.initialize(force)
    return k


def _form(monkeypatch, form):
    if form == "tiles":
        monkeypatch.setenv("AGBNP_HIP_ROWS", "0")
    else:
        monkeypatch.delenv("AGBNP_HIP_ROWS", raising=False)


def _execute(k, pos):
    f = np.zeros(pos.shape)
    return k.execute(pos, f), f


def _report(what, e, f, eo, fo, tol):
    print(f"{what}: |dE|={abs(e - eo):.3e}  max|dF|={float(np.abs(f - fo).max()):.3e}")
    close(e, f, eo, fo, tol)


def _report_single(what, e, f, eo, fo):
    """The single-precision bounds: 2e-6 |E| + 2e-2 kJ/mol, 2e-4 of the largest force."""
    de, df = abs(e - eo), float(np.abs(f - fo).max())
    print(f"{what}: |dE|={de:.3e}  max|dF|={df:.3e}  max|F|={np.abs(fo).max():.3e}")
    assert de < 2e-6 * abs(eo) + 2e-2, (e, eo)
    assert df < 2e-4 * np.abs(fo).max(), (df, np.abs(fo).max())


def _tie_cutoffs(name):
    m = B.TIE_M[name]
    c = B.tie_cutoff(m)
    return {"at the tie": c, "one step above": float(np.nextafter(c, 2.0)), "one step below": float(np.nextafter(c, 0.0)),
            "half a grid step above": B.cutoff_above(m)}


# ---- 1. exact cutoff ties ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["at the tie", "one step above", "one step below"])
@pytest.mark.parametrize("form", FORMS)
def test_fp64_forms_judge_a_cutoff_tie_as_the_oracle_does(gpu_required, monkeypatch, form, which):
    """Snapped 1dwc, 184 pairs exactly at the cutoff (50 heavy-heavy, 92 heavy-H, 42 H-H; across blocks, inside blocks, in GB
    tiles and in GB strips): excluded at c and one step of FP64 below it, included one step above.  The two models are 37 kJ/mol
    and 41 kJ/mol/nm apart: a form that judged the ties the other way, or only some of them (1 / 184 of the jump is 0.2 kJ/mol),
    could not pass FAST_TOL."""
    s = B.boundary_systems()["1dwc_snapped"]
    cutoffs = _tie_cutoffs("1dwc")
    assert abs(_oracle("1dwc_snapped", 1, cutoffs["at the tie"])[0] - _oracle("1dwc_snapped", 1, cutoffs["one step above"])[0]) > 1.0
    eo, fo = _oracle("1dwc_snapped", 1, cutoffs[which])
    _form(monkeypatch, form)
    k = _kernel(s, cutoffs[which], "fast")
    for evaluation in (1, 2):
        e, f = _execute(k, s.pos)
        _report(f"1dwc snapped, fast, {form}, cutoff {which}, evaluation {evaluation}", e, f, eo, fo, FAST_TOL)
    assert k.scalar("rows_on") == (1 if form == "rows" else 0)


def test_single_precision_rows_judge_a_cutoff_tie_as_the_oracle_does(gpu_required, monkeypatch):
    """fast+single on snapped trpcage, nine tied pairs (16.77 kJ/mol, 1.9 per pair, against bounds of 0.024): at c, and at
    sqrt(m + 0.5) / 128.  Not at nextafter(c, 2): (float)gb_cut2 legitimately rounds back onto the tie there -- m / 16384 is a float,
    and one step of FP64 above it is not -- so single precision cannot tell the two cutoffs apart and excludes the ties at both.
    The squared distances themselves are exact in a float relative to any atom.  The GPU's own jump is printed beside the
    oracle's, without a bound."""
    s = B.boundary_systems()["trpcage_snapped"]
    cutoffs = _tie_cutoffs("trpcage")
    _form(monkeypatch, "rows")
    got = {}
    for which in ("at the tie", "half a grid step above"):
        eo, fo = _oracle("trpcage_snapped", 1, cutoffs[which])
        k = _kernel(s, cutoffs[which], "fast+single")
        for evaluation in (1, 2):
            e, f = _execute(k, s.pos)
            _report_single(f"trpcage snapped, fast+single, cutoff {which}, evaluation {evaluation}", e, f, eo, fo)
        assert k.scalar("rows_on") == 1
        got[which] = (e, eo)
    (e0, eo0), (e1, eo1) = got["at the tie"], got["half a grid step above"]
    print(f"trpcage snapped, fast+single: jump across the tie {e1 - e0:.4f} kJ/mol (oracle {eo1 - eo0:.4f})")


@pytest.mark.parametrize("entry", ["execute_device", "execute_openmm double"])
def test_device_entries_judge_a_cutoff_tie_as_the_oracle_does(gpu_required, monkeypatch, entry):
    """The tie logic sits behind every entry: the default row form through execute_device and through execute_openmm (double
    precision: posq holds the grid), at c and one step above, twice each.  execute_device at FAST_TOL; the OpenMM buffers at
    OpenMMContext.check's bounds (fixed-point planes: 1e-6 per evaluation)."""
    torch = pytest.importorskip("torch")
    s = B.boundary_systems()["1dwc_snapped"]
    cutoffs = _tie_cutoffs("1dwc")
    stream = torch.cuda.current_stream().cuda_stream
    _form(monkeypatch, "rows")
    for which in ("at the tie", "one step above"):
        eo, fo = _oracle("1dwc_snapped", 1, cutoffs[which])
        k = _kernel(s, cutoffs[which], "fast")
        k.execute(s.pos, np.zeros((s.n, 3)))  # (the host entry settles capacities: the device entries below withhold nothing)
        for evaluation in (1, 2):
            what = f"1dwc snapped, fast, {entry}, cutoff {which}, evaluation {evaluation}"
            if entry == "execute_device":
                buf = Buffers(torch, s.n)
                buf.load(s.pos)
                torch.cuda.synchronize()
                k.execute_device(*buf.ptrs(), stream)
                assert k.finish(stream) == 0, what
                _report(what, *buf.result(), eo, fo, FAST_TOL)
            else:
                ctx = OpenMMContext(torch, s.n, "double", None)
                ctx.load(s.pos)
                torch.cuda.synchronize()
                ctx.enqueue(k, stream=stream)
                assert k.finish(stream) == 0, what
                ctx.check(eo, fo, 1, what)


# ---- 2. a block box exactly at the cutoff ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["at the gap", "half a grid step above"])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("nh,n", B.BOX_SIZES)
def test_a_block_box_exactly_at_the_cutoff(gpu_required, monkeypatch, nh, n, form, which):
    """Two copies of a snapped piece of 1dwc whose boxes are exactly 0.9375 nm apart, through the one pair of atoms that is
    separated along x alone.  Cutoff 0.9375: the gap2 of the blocks that hold the pair EQUALS cut2 -- culled or walked, no
    cross-copy pair counts.  Cutoff sqrt(14400.5) / 128: the gap2 is 3e-5 nm^2 under cut2 and exactly that pair counts (7 and
    58 kJ/mol): a box that came out a little too large, or a gap compared the wrong way, loses it.  (128, 256): the pair meets in
    a GB strip and a heavy x H tile; (64, 64): in the GB tile (0, 1) and the symmetric heavy tile (0, 1)."""
    name = B.box_pair_name(nh, n)
    s = B.boundary_systems()[name]
    m = B.BOX_GAP_STEPS ** 2
    cutoff = B.tie_cutoff(m) if which == "at the gap" else B.cutoff_above(m)
    eo, fo = _oracle(name, 1, cutoff)
    _form(monkeypatch, form)
    k = _kernel(s, cutoff, "fast")
    for evaluation in (1, 2):
        e, f = _execute(k, s.pos)
        _report(f"{name}, fast, {form}, cutoff {which}, evaluation {evaluation}", e, f, eo, fo, FAST_TOL)
    assert k.scalar("rows_on") == (1 if form == "rows" else 0)


# ---- 3. the last interval of the I4 table ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,form", [("reference", "rows"), ("reference", "tiles"), ("fast", "rows"), ("fast+single", "rows")])
def test_pairs_on_the_last_steps_under_the_tables_reach(gpu_required, monkeypatch, mode, form):
    """Forty atoms of trpcage around a heavy atom A at the origin, and five probes whose squared distance to A is 4 - k 2^-51 as
    the kernels form it: k = 1 and 2, a heavy probe and a hydrogen each, and one at exactly 4 (out).  The FP64 rows index a table of
    15 intervals per type pair, unpadded, with (int)(d2 * rsqrt(d2) * 7.5): a product that rounds up to 2.0 reads the next slice's
    first interval -- Q(0) = 15.6 / nm for the hydrogen probes -- or, from the table's last entry (the heavy probe of A's radius),
    past the table.  The engine's reach stops four steps under 4 for that reason (derive_args, csrc/engine_setup.hip): such a pair
    contributes under 1e-12 where it is still counted (the tiles, whose rows are padded) and nothing where it is not.  Fast mode
    with a cutoff of 2.5 nm has range2 at the tables' reach too; fast+single sees d2 = 4.0f and leaves the pairs out."""
    s = B.boundary_systems()["i4_probes"]
    cutoff = None if mode == "reference" else 2.5
    eo, fo = _oracle("i4_probes", 1, cutoff)
    _form(monkeypatch, form)
    k = _kernel(s, cutoff, mode)
    for evaluation in (1, 2):
        e, f = _execute(k, s.pos)
        what = f"i4 probes, {mode}, {form}, evaluation {evaluation}"
        if mode == "fast+single":
            _report_single(what, e, f, eo, fo)
        else:
            _report(what, e, f, eo, fo, TIGHT)
    assert k.scalar("rows_on") == (1 if form == "rows" else 0)


# ---- 4. exact ties in the sibling order of the tree -------------------------------------------------------------------------------
@pytest.mark.parametrize("version", [0, 1])
@pytest.mark.parametrize("side", B.LATTICE_SIDES)
def test_exact_volume_ties_among_the_siblings_of_a_tree(gpu_required, side, version):
    """Noise-free cubic lattices of identical atoms (64 and 125; the second crosses a 64-heavy block): the candidates of a root tie
    EXACTLY in switched volume, shell by shell, and the tree launch breaks such ties by atom index -- a tie handled wrongly gives two
    children one slot.  The oracle does not depend on the order of these atoms (to 1e-11, pinned on the CPU), so the file's order
    and a fixed permutation both give its numbers at TIGHT, and each other's, un-permuted, at SAME."""
    s = B.boundary_systems()[f"tie_lattice_{side}"]
    perm = B.lattice_permutation(side)
    sp = s.permuted(perm)
    eo, fo = _oracle(s.name, version)
    k, kp = kernel_of(s.params(), version), kernel_of(sp.params(), version)
    for evaluation in (1, 2):
        e, f = _execute(k, s.pos)
        _report(f"{s.name} v{version}, file order, evaluation {evaluation}", e, f, eo, fo, TIGHT)
        e2, f2 = _execute(kp, sp.pos)
        back = np.zeros_like(f2)
        back[perm] = f2
        _report(f"{s.name} v{version}, permuted, evaluation {evaluation}", e2, back, eo, fo, TIGHT)
        _report(f"{s.name} v{version}, permuted against file order, evaluation {evaluation}", e2, back, e, f, SAME)


# ---- 5. far origins -----------------------------------------------------------------------------------------------------------------
FAR_CUTOFF = 1.2  # nm


@pytest.mark.parametrize("entry", ["execute", "execute_openmm double"])
@pytest.mark.parametrize("mode", ["reference", "fast", "fast+single"])
def test_an_origin_thousands_of_nm_away(gpu_required, monkeypatch, mode, entry):
    """Snapped trpcage at its place and moved by (512, -1024, 2048) nm -- exact on the grid, so both geometries have the same
    differences bit for bit.  Each against the oracle at its own positions (reference at TIGHT, fast at FAST_TOL, fast+single at
    its bounds) and the far result against the same context's near one: SAME for FP64, the single bounds for single.  The single
    forms take positions relative to a row's or block's first atom before they round them, precisely so that the origin does not
    matter.  Through execute and through execute_openmm in double precision (forces from the fixed-point planes: compared at
    FIXED_POINT, their resolution, where SAME is asked of the host entry).  OpenMM's single precision is left out: a float posq at
    2048 nm holds steps of 2.4e-4 nm -- a geometry is lost before the engine sees it (this grid alone would survive), so a pass
    there would say nothing.

    What this item found: the pair stages form differences of positions first, which are exact here, but the overlap tree forms the
    centres of products of Gaussians from coordinates, as the reference does (gaussvol.cpp), and at 2048 nm a coordinate rounds at
    2^-42 nm instead of 2^-53: with the caller's coordinates in the trees the FP64 forces moved by 1.41e-09 kJ/mol/nm (execute) and
    1.63e-09 (execute_openmm) between near and far, against SAME = 1e-9; the CPU oracle itself moves by 6.8e-10 (1.1e-11 under a
    64th of the translation, 6.4e-09 under eight times it).  The trees now work relative to the evaluation's first heavy atom
    (build_forest in csrc/tree_kernels.h, prep_atoms in csrc/prep_role.h)."""
    torch = pytest.importorskip("torch")
    s = B.boundary_systems()["trpcage_snapped"]
    far = s.pos + B.FAR_ORIGIN
    cutoff = None if mode == "reference" else FAR_CUTOFF
    tol = TIGHT if mode == "reference" else FAST_TOL
    _form(monkeypatch, "rows")
    k = _kernel(s, cutoff, mode)
    stream = torch.cuda.current_stream().cuda_stream
    if entry != "execute":
        k.execute(s.pos, np.zeros((s.n, 3)))  # (settles capacities, as above)
    got = {}
    for label, pos in (("near", s.pos), ("far", far), ("near again", s.pos)):
        eo, fo = _oracle("trpcage_snapped", 1, cutoff, label.split()[0], pos)
        what = f"trpcage snapped, {mode}, {entry}, {label}"
        if entry == "execute":
            e, f = _execute(k, pos)
        else:
            ctx = OpenMMContext(torch, s.n, "double", None)
            ctx.load(pos)
            torch.cuda.synchronize()
            ctx.enqueue(k, stream=stream)
            if k.finish(stream) != 0:
                # a step of thousands of nm is a long step: withheld once, nothing has arrived, the repeat counts
                assert list(k.withheld()) == [0] and ctx.untouched(), what
                ctx.enqueue(k, stream=stream)
                assert k.finish(stream) == 0, what
            e, f = ctx.energy(), ctx.forces()
        if mode == "fast+single":
            _report_single(what, e, f, eo, fo)
        else:
            _report(what, e, f, eo, fo, tol)
        got[label] = (e, f)
    for label in ("near again", "far"):
        what = f"trpcage snapped, {mode}, {entry}, {label} against near"
        if mode == "fast+single":
            _report_single(what, *got[label], *got["near"])
        else:
            _report(what, *got[label], *got["near"], SAME)
