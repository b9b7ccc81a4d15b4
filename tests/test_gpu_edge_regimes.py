"""GPU box: every entry family at the sizes and in the Born-radius regime that only one path had met (tests/edge_systems.py; pinned
on the CPU by tests/test_edge_systems_oracle.py).

Sizes: test_tiny_and_ragged_systems runs one atom, no heavy atom and 63/64/65 atoms through the host entry point alone.  Here the
device entry points, the OpenMM entry points (slots through hslot, padding to 32), the energy-only instantiations and the group
kernels (per-member offsets into shared launches) meet systems of exactly 64 / 128 / 256 heavy atoms and 256 / 512 atoms, one
beside those, a single atom, and no heavy atom at all (nhb == 0: no forest, no tree workgroup).

Born radii: born_radius() in csrc/row_kernels.h has the two arms of ReferenceAGBNPKernels.cpp:41-55 -- beta < 0: 1/B = 1/2 nm and
f' = 0; otherwise sqrt(a^2 + beta^2).  No other input of the suite has a Born radius beyond 0.75 nm: the first arm, f' = 0 in
bw_alpha and bw_beta, and the far-strip bound of gb_strip with Born radii at their cap run here only.

The reference is the CPU oracle at the positions the engine sees; the tolerances are those of tests/gpu_helpers.py, of
tests/openmm_context.py and the fast-mode bar of tests/test_gpu_parity.py.  Every comparison prints |dE| and max|dF| first."""
import numpy as np
import pytest

import openmm_agbnp_plugin_amd as P
from oracle import Oracle
from tests.edge_systems import NAMES, STRIP_NAMES, edge_systems, size_edge_name
from tests.gpu_helpers import SAME, TIGHT, Buffers, close, energy_close, execute_group, kernel_of
from tests.gpu_helpers import five  # noqa: F401
from tests.openmm_context import ENERGY_SLOT, OpenMMContext
from tests.test_gpu_parity import FAST_TOL, assert_close

pytestmark = pytest.mark.gpu

SENTINEL, PLANE_SENTINEL = -1234.5678, 7
SINGLE_CONTEXT_FAMILIES = ("execute", "energy", "execute_device", "energy_device", "execute_openmm double", "energy_openmm double",
                           "execute_openmm mixed", "energy_openmm mixed")
GROUP_FAMILIES = ("execute_group", "energy_group", "execute_group_host", "energy_group_host")


def _report(what, e, f, eo, fo, tol=TIGHT):
    """Prints the deviations, then compares: close() with forces, energy_close() without."""
    df = 0.0 if f is None else float(np.abs(f - fo).max())
    print(f"{what}: |dE|={abs(e - eo):.3e}  max|dF|={df:.3e}")
    if f is None:
        energy_close(e, eo, tol)
    else:
        close(e, f, eo, fo, tol)


def _energy_openmm(k, ctx, posq, corr, stream):
    k.energy_openmm(posq.data_ptr(), ctx.precision == "double", corr.data_ptr() if corr is not None else 0, ctx.index.data_ptr(), ctx.padded,
                    ctx.ebuf.data_ptr(), ctx.energy_is_double, ENERGY_SLOT, stream)


@pytest.mark.parametrize("version", [0, 1])
@pytest.mark.parametrize("name", NAMES)
def test_every_family_on_every_edge_system(gpu_required, five, name, version):
    """One kernel; the eight single-context families in turn at the file geometry, then at jittered(1), called the way
    test_every_entry_family_in_turn_leaves_nothing_behind calls them.  The OpenMM entry points run behind two contexts' buffers
    (double; mixed), atoms shuffled and padded to 32.  FP64 targets at TIGHT, the planes and the energy buffer through
    OpenMMContext.check; an energy-only step leaves a sentinel-filled force buffer or plane as loaded; nothing is withheld.  (No
    launch count: a system without heavy atoms has no tree work.)"""
    torch = pytest.importorskip("torch")
    s = edge_systems()[name]
    oracle = Oracle(*s.params(), version=version)
    k = kernel_of(s.params(), version)
    ctxs = {precision: OpenMMContext(torch, s.n, precision, oracle) for precision in ("double", "mixed")}
    for ctx in ctxs.values():
        assert ctx.padded % 32 == 0 and ctx.padded >= s.n
        assert s.n < 3 or (ctx.order != np.arange(s.n)).any()  # (slot == index would hide a wrong map)
    buf = Buffers(torch, s.n)
    stream = torch.cuda.current_stream().cuda_stream
    for label, pos in (("file", s.pos), ("jittered", s.jittered(1))):
        for family in SINGLE_CONTEXT_FAMILIES:
            what = f"{name} v{version} {label} {family}"
            energy_only = family.startswith("energy")
            if "openmm" in family:
                ctx = ctxs[family.split()[1]]
                hi, lo, seen = ctx.host_arrays(pos)
                posq = torch.tensor(hi, device=ctx.dev)
                corr = torch.tensor(lo, device=ctx.dev) if lo is not None else None
                eo, fo = oracle.execute(seen)
                if energy_only:
                    ctx.fixed.fill_(PLANE_SENTINEL)
                    torch.cuda.synchronize()
                    _energy_openmm(k, ctx, posq, corr, stream)
                    assert k.finish(stream) == 0, what
                    assert (ctx.fixed == PLANE_SENTINEL).all(), "an energy-only evaluation wrote to the fixed-point planes"
                    _report(what, ctx.energy(), None, eo, None)
                    ctx.clear()
                else:
                    ctx.enqueue(k, posq, corr, stream)
                    assert k.finish(stream) == 0, what
                    ctx.check(eo, fo, 1, what)
                continue
            eo, fo = oracle.execute(pos)
            if family == "execute":
                f = np.zeros((s.n, 3))
                e = k.execute(pos, f)
            elif family == "energy":
                e, f = k.energy(pos), None
            else:
                buf.load(pos, SENTINEL if energy_only else 0.0)
                torch.cuda.synchronize()
                if energy_only:
                    k.energy_device(buf.pos.data_ptr(), buf.ene.data_ptr(), stream)
                else:
                    k.execute_device(*buf.ptrs(), stream)
                assert k.finish(stream) == 0, what
                e, f = buf.result()
                if energy_only:
                    assert (f == SENTINEL).all(), "an energy-only evaluation wrote to the caller's force buffer"
                    f = None
            assert k.finish(stream) == 0, what
            _report(what, e, f, eo, fo)


def _member_sets():
    table = edge_systems()
    size = lambda nh, n: table[size_edge_name(nh, n)]  # noqa: E731
    return {
        "one atom, a full block, one beside two blocks": [size(0, 1), size(64, 64), size(129, 257)],
        "no heavy atom, the clamp cluster, one heavy atom": [size(0, 32), table["born_clamp"], size(1, 1)],
        "three of (128, 256)": [size(128, 256)] * 3,
    }


@pytest.mark.parametrize("members", list(_member_sets()))
def test_groups_of_edge_members(gpu_required, five, members):
    """execute_group, energy_group, execute_group_host and energy_group_host on members of edge sizes, every member on a jittered
    geometry of its own per call: each member's result is its oracle's at TIGHT, and for the two execute families also that of a
    twin context run alone through execute_device, to SAME.  (Whether the members share launches is the engine's choice.)"""
    torch = pytest.importorskip("torch")
    systems = _member_sets()[members]
    oracles = [Oracle(*s.params(), version=1) for s in systems]
    ks = [kernel_of(s.params()) for s in systems]
    twins = [kernel_of(s.params()) for s in systems]
    bufs = [Buffers(torch, s.n) for s in systems]
    tb = [Buffers(torch, s.n) for s in systems]
    stream = torch.cuda.current_stream().cuda_stream
    for step, family in enumerate(GROUP_FAMILIES):
        energy_only = family.startswith("energy")
        geoms = [s.jittered(10 * m + step) for m, s in enumerate(systems)]
        want = [o.execute(g) for o, g in zip(oracles, geoms)]
        for b, g in zip(bufs, geoms):
            b.load(g, SENTINEL if energy_only else 0.0)
        torch.cuda.synchronize()
        if family == "execute_group":
            execute_group(ks, bufs, stream)
        elif family == "energy_group":
            P.energy_group(ks, [b.pos.data_ptr() for b in bufs], [b.ene.data_ptr() for b in bufs], stream)
        elif family == "execute_group_host":
            fs = [np.zeros((s.n, 3)) for s in systems]
            got = list(zip(P.execute_group_host(ks, geoms, fs), fs))
        else:
            got = [(e, None) for e in P.energy_group_host(ks, geoms)]
        assert [k.finish(stream) for k in ks] == [0] * len(ks), family
        if "host" not in family:
            got = [b.result() for b in bufs]
            if energy_only:
                assert all((f == SENTINEL).all() for _, f in got), "an energy-only evaluation wrote to a caller's force buffer"
                got = [(e, None) for e, _ in got]
        for m, ((e, f), (eo, fo)) in enumerate(zip(got, want)):
            _report(f"{members}: {family}, member {m} ({systems[m].name})", e, f, eo, fo)
        if not energy_only:
            for m, (tw, t, g) in enumerate(zip(twins, tb, geoms)):
                t.load(g)
                tw.execute_device(*t.ptrs(), stream)
                assert tw.finish(stream) == 0
                _report(f"{members}: {family}, member {m} against its twin alone", *got[m], *t.result(), tol=SAME)


def test_the_born_clamp_through_the_diagnostics(gpu_required, five):
    """The Born radii themselves: with the diagnostics on, the engine's born, scale and selfvol_vdw vectors are the oracle's to
    1e-12 (the bar of test_diagnostic_vectors) and at least eight of its Born radii are EXACTLY 2 nm.  Then the file geometry and
    jittered(0..3) -- the capped atoms number 11, 10, 11, 10, 10: an atom crosses beta = 0 between evaluations -- queued through
    execute_device before anybody reads the log, on that kernel and on a fresh one (which stays in the five-launch mode): the
    accumulated sums are the oracle's at 5 * TIGHT."""
    torch = pytest.importorskip("torch")
    s = edge_systems()["born_clamp"]
    oracle = Oracle(*s.params(), version=1)
    stream = torch.cuda.current_stream().cuda_stream
    k = kernel_of(s.params())
    k.set_diagnostics(True)
    f = np.zeros((s.n, 3))
    e = k.execute(s.pos, f)
    eo, fo = oracle.execute(s.pos)
    _report("born_clamp with diagnostics", e, f, eo, fo)
    for vector in ("born", "scale", "selfvol_vdw"):
        got, want = k.vector(vector), oracle.vector(vector)
        print(f"born_clamp {vector}: max deviation {np.abs(got - want).max():.3e}")
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
    born = k.vector("born")
    assert (born == 2.0).sum() >= 8
    np.testing.assert_array_equal(born == 2.0, oracle.vector("born") == 2.0)
    geoms = [s.pos] + [s.jittered(step) for step in range(4)]
    want = [oracle.execute(g) for g in geoms]
    we, wf = sum(w[0] for w in want), sum(w[1] for w in want)
    for what, kernel in (("diagnostics on", k), ("five-launch mode", kernel_of(s.params()))):
        bufs = [Buffers(torch, s.n) for _ in geoms]  # positions of their own per queued evaluation, one force and energy target
        for b, g in zip(bufs, geoms):
            b.load(g)
        torch.cuda.synchronize()
        for b in bufs:
            kernel.execute_device(b.pos.data_ptr(), bufs[0].frc.data_ptr(), bufs[0].ene.data_ptr(), stream)
        assert kernel.finish(stream) == 0, (what, list(kernel.withheld()))
        e, f = bufs[0].result()
        print(f"born_clamp, five queued evaluations ({what}): |dE|={abs(e - we):.3e}  max|dF|={np.abs(f - wf).max():.3e}")
        energy_close(e, we, 5 * TIGHT)
        assert np.abs(f - wf).max() < 5 * TIGHT


@pytest.mark.parametrize("name", ["born_clamp_pair_24", "born_clamp_pair_27"] + list(STRIP_NAMES))
def test_far_strips_with_capped_born_radii(gpu_required, five, monkeypatch, name):
    """The protocol of test_far_strips_of_the_gb_stage_are_coulomb_to_rounding with Born radii AT their cap, where the bound
    sqrt(4 * 60 ln2 * Bmax_I * Bmax_J) is 25.8 nm: two copies of born_clamp 24 and 27 nm apart, and the three-block systems
    (tests/edge_systems.py: born_clamp_strip) whose blocks {0, 1} and 2 have gaps of 12, 24 and 27 nm -- the pairs are 42 atoms,
    one block, and launch no strip; the three-block systems launch one.  AGBNP_HIP_GB_FAR = 1 and 0 both give the oracle's numbers
    at TIGHT and each other's to 1e-9.  No counter exposes the far strips; the equality is the check, and it is a sharp one at
    12 nm: there a Coulomb-only strip is off by 3.6e-5 kJ/mol (exp(-d^2 / 4 B_i B_j) = 1e-4), and a bound made of Born radii under
    0.93 nm -- any but capped ones -- takes the strip for far.  At 24 nm the exponential is 2^-52 and either loop gives the same
    numbers; at 27 nm the Coulomb-only loop runs with capped radii in its prologue."""
    s = edge_systems()[name]
    pos = s.jittered(5, sigma=0.003)
    out = {}
    for far in ("1", "0"):
        monkeypatch.setenv("AGBNP_HIP_GB_FAR", far)
        ctx = P.AGBNPContext(P.AGBNPForce.from_arrays(*s.params(), version=1))
        ctx.setPositions(s.pos)
        ctx.getState()
        ctx.setPositions(pos)
        out[far] = ctx.getState()
    eo, fo = Oracle(*s.params(), version=1).execute(pos)
    _report(f"{name}, far-strip test on", *out["1"], eo, fo)
    _report(f"{name}, far-strip test off", *out["0"], eo, fo)
    de, df = abs(out["1"][0] - out["0"][0]), float(np.abs(out["1"][1] - out["0"][1]).max())
    print(f"{name}, on against off: |dE|={de:.3e}  max|dF|={df:.3e}")
    assert de < 1e-9 * max(1.0, abs(eo) * 1e-3) and df < 1e-9


@pytest.mark.parametrize("cutoff", [0.3, 1.2])
def test_fast_mode_on_the_born_clamp(gpu_required, five, cutoff):
    """AGBNP_HIP_MODE_FAST (CutoffNonPeriodic) against the oracle's cutoff switch, at the bar of
    test_fast_mode_matches_the_cutoff_oracle, on the file geometry and a jittered one: the row form of every pair stage, GB
    included, with capped Born radii (cutoff 1.2 nm holds the whole cluster: eleven capped atoms as without a cutoff; at 0.3 nm
    the truncated descreening sums leave one)."""
    s = edge_systems()["born_clamp"]
    force = P.AGBNPForce.from_arrays(*s.params(), version=1)
    force.setNonbondedMethod(P.AGBNPForce.CutoffNonPeriodic)
    force.setCutoffDistance(cutoff)
    k = P.HipCalcAGBNPForceKernel(mode="fast")
    k.initialize(force)
    oracle = Oracle(*s.params(), version=1, cutoff=cutoff)
    for label, pos in (("file", s.pos), ("jittered", s.jittered(1, sigma=0.004))):
        f = np.zeros((s.n, 3))
        e = k.execute(pos, f)
        eo, fo = oracle.execute(pos)
        if cutoff == 1.2:
            assert (oracle.vector("born") == 2.0).sum() >= 1
        print(f"born_clamp fast mode, cutoff {cutoff}, {label}: |dE|={abs(e - eo):.3e}  max|dF|={np.abs(f - fo).max():.3e}")
        assert_close(e, f, eo, fo, tol=FAST_TOL)


ROW_EDGE_CUTOFF = 1.0  # nm


@pytest.mark.parametrize("mode", ["fast", "fast+single"])
@pytest.mark.parametrize("nh,n", [(65, 65), (63, 255), (129, 257)])
def test_row_form_on_ragged_sizes(gpu_required, five, nh, n, mode):
    """The row form of all three pair stages -- in FP64 (fast) and with single-precision pair terms (fast+single) -- at sizes
    that leave the last row group short (65, 255 and 257 atoms: groups of four) and the last 64-atom block part filled, against
    the oracle's cutoff switch at 1.0 nm: the file geometry, then one drawn as test_fast_single_mode_rows_against_the_cutoff_oracle
    draws it, which rebuilds the lists.  fast at FAST_TOL; fast+single at that test's single-precision bounds, 2e-6 |E| + 2e-2
    and 2e-4 of the largest force."""
    s = edge_systems()[size_edge_name(nh, n)]
    force = P.AGBNPForce.from_arrays(*s.params(), version=1)
    force.setNonbondedMethod(P.AGBNPForce.CutoffNonPeriodic)
    force.setCutoffDistance(ROW_EDGE_CUTOFF)
    k = P.HipCalcAGBNPForceKernel(mode=mode)
    k.initialize(force)
    oracle = Oracle(*s.params(), version=1, cutoff=ROW_EDGE_CUTOFF)
    rng = np.random.default_rng(9)
    for label, pos in (("file", s.pos), ("drawn", s.pos + rng.normal(0.0, 0.04, s.pos.shape))):
        f = np.zeros((s.n, 3))
        e = k.execute(pos, f)
        eo, fo = oracle.execute(pos)
        de, df = abs(e - eo), float(np.abs(f - fo).max())
        print(f"{size_edge_name(nh, n)}, {mode}, {label}: |dE|={de:.3e}  max|dF|={df:.3e}  max|F|={np.abs(fo).max():.3e}")
        if mode == "fast":
            close(e, f, eo, fo, FAST_TOL)
        else:
            assert de < 2e-6 * abs(eo) + 2e-2, (e, eo)
            assert df < 2e-4 * np.abs(fo).max(), (df, np.abs(fo).max())
    assert k.scalar("rows_on") == 1
