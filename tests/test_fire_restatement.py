"""The CPU restatement of the FIRE minimiser's two launches (tests/fire_restatement.py) on the CPU: its synthetic sequences
meet every branch of the back half with verdicts that do not hang on the last bits, it agrees with a plain double-precision
FIRE written independently of it, and the minimiser built on it finds a known minimum.  Nothing here needs a device."""
import numpy as np
import pytest

from tests import fire_restatement as fr
from tests import md_restatement as mr
from tests.md_kernel_harness import CASES, assert_same_state, same_bits

LD = np.longdouble


def start(n, R):
    """The sequence's start, as minimise() starts: tethers, then the stand-in evaluation with its energy."""
    state, y0 = fr.synthetic_state(n, R)
    return mr.evaluated(mr.tethers(state, 0), y0), y0


def sequence(n, R, iterations=fr.ITERATIONS):
    """The synthetic sequence of the kernel tests through the restatement: per iteration (state before, bounds of the back
    half, state behind it, masks of the capped atoms, state behind the front half).  The evaluation of iteration VOID_AT is
    withheld for replica 0: its energy word is zero."""
    state, y0 = start(n, R)
    out = []
    for it in range(iterations):
        if it == fr.VOID_AT:
            state["energy"][0] = 0.0
        bounds, capped = {}, []
        judged = fr.back(state, 0, bounds)
        moved = fr.front(judged, 0, capped)
        out.append((state, bounds, judged, capped, moved))
        state = mr.evaluated(moved, y0)
    return out


@pytest.mark.parametrize("n,R,iterations", [(n, R, fr.ITERATIONS) for n, R in CASES] + [(65537, 2, 12)])  # (the GPU test's sequences)
def test_the_synthetic_sequence_meets_every_branch(n, R, iterations):
    """About the test's own inputs: F.w > 0 with npos at most n_min and beyond it, F.w <= 0, a dt_max clamp, a void iteration,
    from 63 atoms on an atom whose move is capped beside one whose move is not, and for R >= 2 a replica that converges while
    the others go on; and no verdict hangs on the last bits: |F.w| > 1e-6 sum_i |F_i.w_i| and |fmax - tolerance| > 1e-6 tolerance
    at every judged evaluation."""
    seen, clamp, cap_some, cap_not_all, lone = set(), False, False, False, False
    for before, bounds, judged, capped, moved in sequence(n, R, iterations):
        for r in range(R):
            branch = bounds["branch"][r]
            if branch in ("positive", "negative", "done"):
                assert abs(judged["fmax"][r] - fr.TOLERANCE) > 1e-6 * fr.TOLERANCE, (r, judged["fmax"][r])
            if branch in ("positive", "negative"):
                assert abs(bounds["P"][r]) > 1e-6 * bounds["absP"][r], (r, bounds["P"][r], bounds["absP"][r])
                assert (branch == "positive") == (bounds["P"][r] > 0)
            if branch == "positive":
                branch += " beyond n_min" if judged["npos"][r] > fr.CONSTANTS["n_min"] else ""
                clamp |= judged["fdt"][r] == fr.DT_MAX and before["fdt"][r] * fr.CONSTANTS["f_inc"] > fr.DT_MAX
            seen.add(branch)
            if capped[r] is not None:
                cap_some |= bool(capped[r].any())
                cap_not_all |= bool(capped[r].any() and not capped[r].all())
        lone |= any(b == "done" for b in bounds["branch"]) and any(b in ("positive", "negative") for b in bounds["branch"])
    assert {"positive", "positive beyond n_min", "negative", "void"} <= seen, seen
    assert clamp
    if n >= 63:
        assert cap_some and cap_not_all
    if R >= 2:
        assert lone and "converged" in seen


def plain_back(s, part):
    """The back half in plain double numpy, written from the kernel's header comment without the restatement: returns the words
    it decides as a dict per replica."""
    out = []
    for r in range(len(s["x"])):
        F, W = s["f"][r], s["w"][r]
        P, Q, S, M = float((F * W).sum()), float((F * F).sum()), float((W * W).sum()), float((F * F).sum(axis=1).max())
        e = float(s["energy"][r])
        d = dict(dt=s["fdt"][r], alpha=s["alpha"][r], npos=int(s["npos"][r]), iterations=int(s["iterations"][r]),
                 converged=int(s["converged"][r]), voids=int(s["voids"][r]), move=0.0, a=None, b=None, E=None, fmax=None)
        if e == 0.0 or not np.isfinite(e) or not np.isfinite(Q):
            d["voids"] += 1
        elif d["converged"]:
            pass
        else:
            d["E"], d["fmax"] = float(s["parts"][part][r].sum()) + e, np.sqrt(M)
            d["iterations"] += 1
            if d["fmax"] < s["tolerance"]:
                d["converged"] = 1
            elif P > 0.0:
                d["npos"] += 1
                d["a"], d["b"], d["move_dt"], d["move"] = 1.0 - d["alpha"], d["alpha"] * np.sqrt(S / Q), d["dt"], 1.0
                if d["npos"] > s["n_min"]:
                    d["dt"], d["alpha"] = min(d["dt"] * s["f_inc"], s["dt_max"]), d["alpha"] * s["f_alpha"]
            else:
                d["npos"], d["dt"], d["alpha"] = 0, d["dt"] * s["f_dec"], s["alpha0"]
                d["a"], d["b"], d["move_dt"], d["move"] = 0.0, 0.0, d["dt"], 1.0
        out.append(d)
    return out


@pytest.mark.parametrize("n,R", [(65, 2), (257, 3), (513, 16)])
def test_the_restatement_is_a_plain_double_fire(n, R):
    """Every back half of the sequence against `plain_back` on the same state.  dt, alpha, npos, iterations, converged, voids
    and the coefficient a, each one correctly rounded operation on doubles: bit for bit.  b, the logged energy and fmax come out
    of sums: at the summation bounds the restatement reports.  The move of the plain FIRE (numpy double) reproduces the front
    half's x and w at 1e-15 nm and 1e-12 nm/ps."""
    for before, bounds, judged, capped, moved in sequence(n, R):
        for r, d in enumerate(plain_back(before, 0)):
            assert np.float64(d["dt"]).tobytes() == judged["fdt"][r].tobytes() and np.float64(d["alpha"]).tobytes() == judged["alpha"][r].tobytes()
            assert (d["npos"], d["iterations"], d["converged"], d["voids"]) == tuple(int(judged[key][r]) for key in
                                                                                      ("npos", "iterations", "converged", "voids"))
            assert d["move"] == judged["coef"][r, 3]
            if d["move"]:
                assert np.float64(d["a"]).tobytes() == judged["coef"][r, 0].tobytes()
                assert np.float64(d["move_dt"]).tobytes() == judged["coef"][r, 2].tobytes()
                assert abs(d["b"] - judged["coef"][r, 1]) <= bounds["b"][r]
                m = before["mass"][:, None]
                w = d["a"] * before["w"][r] + d["b"] * before["f"][r]
                w = w + (d["move_dt"] / m) * before["f"][r]
                step = d["move_dt"] * w
                length = np.sqrt((step * step).sum(axis=1))[:, None]
                scale = np.where(length > before["max_move"], before["max_move"] / np.maximum(length, 1e-300), 1.0)
                assert np.abs(before["x"][r] + step * scale - moved["x"][r]).max() < 1e-15
                assert np.abs(w * scale - moved["w"][r]).max() < 1e-12
                assert np.sqrt(((moved["x"][r] - before["x"][r]) ** 2).sum(axis=1)).max() <= before["max_move"] * (1.0 + 1e-12)
            else:
                assert same_bits(moved["x"][r], before["x"][r]) and same_bits(moved["w"][r], before["w"][r])
            if d["E"] is not None:
                slot = fr.FGUARD + r * fr.FCAP + int(before["iterations"][r])
                assert abs(d["fmax"] - judged["fmax"][r]) <= bounds["fmax"][r]
                if before["iterations"][r] < fr.FCAP:
                    assert abs(d["E"] - judged["log_e"][slot]) <= bounds["E"][r] and judged["log_fmax"][slot] == judged["fmax"][r]
        assert np.all(judged["energy"] == 0.0) and np.all(judged["arrived"] == 0)


def test_what_a_launch_must_not_write_stays():
    """Through the whole sequence of (257, 3): v, step, log_pe, log_ke, last, acc, done and parts[1] keep their bits; the back
    half writes neither x, w, f nor parts[0], the front half none of the minimiser's state words; the logs change only at the
    iteration's slot where it lies inside the capacity (replica 1 starts at slot 10 of 16, replica 2 beyond 2^32), the guards never."""
    for before, bounds, judged, capped, moved in sequence(257, 3):
        for key in ("v", "step", "log_pe", "log_ke", "last", "acc", "done", "x0", "mass", "hdt_m", "kT", "seeds"):
            assert same_bits(before[key], judged[key]) and same_bits(before[key], moved[key]), key
        assert same_bits(before["parts"][1], moved["parts"][1])
        assert_same_state(before, judged, but=("energy", "arrived", "fpart", "coef", "fdt", "alpha", "npos", "iterations", "converged", "voids",
                                               "fmax", "log_e", "log_fmax"))
        assert_same_state(judged, moved, but=("x", "w", "f", "parts"))
        for key in ("log_e", "log_fmax"):
            changed = list(np.flatnonzero(before[key].view(np.uint64) != judged[key].view(np.uint64)))
            slots = [fr.FGUARD + r * fr.FCAP + int(before["iterations"][r]) for r in range(3)
                     if bounds["branch"][r] in ("positive", "negative", "done") and before["iterations"][r] < fr.FCAP]
            assert changed == slots
    # replica 0 had one void iteration, replica 1 none, and replica 2 stopped counting when it converged
    assert list(moved["iterations"][:2]) == [fr.ITERATIONS - 1, 10 + fr.ITERATIONS] and list(moved["converged"]) == [0, 0, 1]
    assert (1 << 32) + 3 < moved["iterations"][2] < (1 << 32) + 3 + fr.ITERATIONS


def test_a_void_iteration_changes_nothing_but_the_count():
    """The energy word zero, NaN or infinite, or a force that is not finite: voids + 1, move = 0, energy and arrived handed back as zeros, the partials; the
    front half behind it rewrites f and the tether partials and leaves x and w alone."""
    state, y0 = start(65, 2)
    state = mr.evaluated(fr.front(fr.back(state, 0), 0), y0)
    for word in (0.0, -0.0, np.nan, np.inf):
        void = fr.copy_state(state)
        void["energy"][1] = word
        judged = fr.back(void, 0)
        assert list(judged["voids"]) == [0, 1] and judged["coef"][1, 3] == 0.0 and judged["coef"][0, 3] == 1.0
        assert_same_state(void, judged, but=("energy", "arrived", "fpart", "coef", "voids", "fdt", "alpha", "npos", "iterations", "fmax",
                                             "log_e", "log_fmax"))
        for key in ("fdt", "alpha", "npos", "iterations", "fmax"):
            assert same_bits(void[key][1:], judged[key][1:]), key
        assert same_bits(void["coef"][1, :3], judged["coef"][1, :3])
        moved = fr.front(judged, 0)
        assert same_bits(moved["x"][1], void["x"][1]) and same_bits(moved["w"][1], void["w"][1])
        assert not same_bits(moved["x"][0], void["x"][0])
    # a force that is not a number beside a finite energy word is void as well (max |F_i|^2 alone would not see it) ...
    for word in (np.nan, np.inf):
        void = fr.copy_state(state)
        void["f"][1, 3, 0] = word
        judged = fr.back(void, 0)
        assert list(judged["voids"]) == [0, 1] and judged["coef"][1, 3] == 0.0 and list(judged["converged"]) == [0, 0]
        assert judged["iterations"][1] == void["iterations"][1] and same_bits(judged["fmax"][1:], void["fmax"][1:])
    # ... and a converged replica counts a withheld evaluation like any other, and stays converged
    void = fr.copy_state(state)
    void["converged"][1], void["energy"][1] = 1, 0.0
    judged = fr.back(void, 0)
    assert list(judged["voids"]) == [0, 1] and list(judged["converged"]) == [0, 1] and judged["coef"][1, 3] == 0.0
    assert judged["iterations"][1] == void["iterations"][1]


def test_a_function_leaves_its_argument_alone():
    state, _ = start(5, 2)
    keep = fr.copy_state(state)
    judged = fr.back(state, 0, {})
    assert_same_state(state, keep)
    keep = fr.copy_state(judged)
    fr.front(judged, 0, [])
    assert_same_state(judged, keep)


def test_the_cpu_minimiser_finds_the_stand_ins_minimum():
    """fire_restatement.minimise (the reference of tests/test_gpu_minimise.py) on tethers + the harmonic stand-in, 65 atoms: it
    converges, the forces recomputed at its final positions are below the tolerance, the final positions are within
    tolerance / (k + k2) of the analytic minimum, the logged energy falls from its first value to within 1e-9 of the minimum's,
    and no move exceeded max_move although the cap was in use."""
    base = mr.synthetic_state(65, 1)
    y0 = mr.standin_anchor(base)
    x = base["x0"] + 0.05 * np.sin(37.0 * base["x0"])

    def evaluate(pos):
        F, E = mr.standin(pos[None], y0)
        return float(E[0]), F[0]

    tol = 1e-3
    out = fr.minimise(evaluate, x, base["x0"], base["mass"], base["k"], tolerance=tol, max_iterations=2000, max_move=0.01)
    assert out["converged"] and out["iterations"] < 2000 and out["capped"] > 0
    total = -base["k"] * (out["x"] - base["x0"]) + evaluate(out["x"])[1]
    fmax = np.sqrt((total * total).sum(axis=1)).max()
    assert fmax < tol and abs(fmax - out["fmax"]) < 1e-9
    best = fr.standin_minimum(base, y0)
    assert np.abs(out["x"] - best).max() <= tol / (base["k"] + mr.K2)
    e_min = 0.5 * base["k"] * ((best - base["x0"]) ** 2).sum() + evaluate(best)[0]
    assert out["log_e"][0] > e_min + 100.0 and abs(out["energy"] - e_min) < 1e-9 and out["energy"] == out["log_e"][-1]
    print(f"{out['iterations']} iterations, {out['capped']} with a capped atom, E {out['log_e'][0]:.4f} -> {out['energy']:.6f} (minimum {e_min:.6f})")
