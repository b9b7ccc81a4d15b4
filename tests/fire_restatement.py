"""A CPU restatement of the two launches of the FIRE minimiser (agbnp_md_fire_back, agbnp_md_fire_front of
openmm_agbnp_plugin_amd/csrc/md_kernels.hip), written from that file's header comment in numpy.longdouble in the style of
tests/md_restatement.py, the synthetic inputs the tests of the kernels share, and the same FIRE as a CPU minimiser around any
evaluation (the reference of tests/test_gpu_minimise.py).  A plain module: tests/test_fire_restatement.py checks it on the CPU,
tests/test_gpu_fire_kernels.py judges the kernels by it.

The state is md_restatement's dict (x, f, x0, mass, k, energy, parts, ... and every word the minimiser must NOT touch: v, step,
log_pe, log_ke, last, acc, done) with the minimiser's words added:

  w [R][n][3];  fdt, alpha, fmax [R];  npos, converged, voids [R] (int32);  iterations [R] (int64);  arrived [R] (uint32)
  coef [R][4] {a, b, dt, move};  fpart [R][blocks(n)][4] {sum F.w, sum F.F, sum w.w, max |F_i|^2}
  log_e, log_fmax: flat, `fguard` guard words, [R][fcap], `fguard` guard words;  fcap, fguard
  dt_max, f_inc, f_dec, alpha0, f_alpha, n_min, tolerance, max_move

back() and front() take a state and return the predicted state after ONE launch, leaving their argument alone.  What the
kernel forms by one correctly rounded IEEE operation on doubles (dt, alpha, the coefficient a) is formed in double here and
expected bit for bit, as are the integer words; what comes out of a sum (the partials, b, the logged energy, fmax) is formed in
long double, rounded where the kernel stores a double, and compared at the summation bound (terms - 1) 2^-52 sum |term|, which
back() reports on request."""
import numpy as np

from tests import md_restatement as mr

LD = np.longdouble
BLOCK = mr.BLOCK
EPS = 2.0 ** -52
blocks = mr.blocks
copy_state = mr.copy_state


def _per_block(per_atom, op):
    n = len(per_atom)
    return np.array([op(per_atom[b * BLOCK:(b + 1) * BLOCK]) for b in range(blocks(n))], dtype=LD)


def back(state, part, bounds=None):
    """agbnp_md_fire_back: judge the evaluation in f / energy, the tether partials read are parts[part].  `bounds`, a dict,
    receives per replica what the tests need to judge the sums: the summation bounds of fpart [R][blocks][4], b, E and fmax, the
    sums P = F.w and absP = sum_i |F_i . w_i|, and the branch taken ("converged", "void", "done", "positive", "negative")."""
    out = copy_state(state)
    R, n = state["x"].shape[:2]
    nb, cap, guard = blocks(n), int(state["fcap"]), int(state["fguard"])
    if bounds is not None:
        bounds.update(fpart=np.zeros((R, nb, 4)), b=np.zeros(R), E=np.zeros(R), fmax=np.zeros(R), P=np.zeros(R), absP=np.zeros(R),
                      branch=[None] * R)
    for r in range(R):
        F, W = state["f"][r].astype(LD), state["w"][r].astype(LD)
        p, q, s = (F * W).sum(axis=1), (F * F).sum(axis=1), (W * W).sum(axis=1)
        sums = np.stack([_per_block(p, np.sum), _per_block(q, np.sum), _per_block(s, np.sum), _per_block(q, np.nanmax)], axis=1)
        out["fpart"][r] = sums.astype(np.float64)
        stored = out["fpart"][r].astype(LD)
        P, Q, S, M = stored[:, 0].sum(), stored[:, 1].sum(), stored[:, 2].sum(), stored[:, 3].max()
        T = state["parts"][part][r].astype(LD).sum()
        e = state["energy"][r]
        out["energy"][r], out["arrived"][r] = 0.0, 0
        if bounds is not None:
            count = _per_block(np.ones(n, dtype=LD), np.sum)
            for j, terms in enumerate((np.abs(F * W), F * F, W * W)):
                bounds["fpart"][r, :, j] = np.array((3 * count - 1) * EPS * _per_block(terms.sum(axis=1), np.sum), dtype=np.float64)
            bounds["fpart"][r, :, 3] = np.array(2 * EPS * sums[:, 3], dtype=np.float64)
            bounds["P"][r], bounds["absP"][r] = float(P), float(np.abs(p).sum())
        if e == 0.0 or not np.isfinite(e) or not np.isfinite(Q):
            out["voids"][r] += 1
            out["coef"][r, 3] = 0.0
            branch = "void"
        elif state["converged"][r] != 0:
            out["coef"][r, 3] = 0.0
            branch = "converged"
        else:
            E, fm = np.float64(T + LD(e)), np.float64(np.sqrt(M))
            it = int(state["iterations"][r])
            if it < cap:
                out["log_e"][guard + r * cap + it], out["log_fmax"][guard + r * cap + it] = E, fm
            out["fmax"][r] = fm
            out["iterations"][r] = it + 1
            dt, alpha = np.float64(state["fdt"][r]), np.float64(state["alpha"][r])
            b = np.float64(0.0)
            if fm < state["tolerance"]:
                out["converged"][r] = 1
                out["coef"][r, 3] = 0.0
                branch = "done"
            elif P > 0:
                npos = int(state["npos"][r]) + 1
                out["npos"][r] = npos
                b = np.float64(LD(alpha) * np.sqrt(S / Q)) if Q > 0 else np.float64(0.0)
                out["coef"][r] = np.float64(1.0) - alpha, b, dt, 1.0
                if npos > int(state["n_min"]):
                    out["fdt"][r] = min(dt * np.float64(state["f_inc"]), np.float64(state["dt_max"]))
                    out["alpha"][r] = alpha * np.float64(state["f_alpha"])
                branch = "positive"
            else:
                cut = dt * np.float64(state["f_dec"])
                out["npos"][r], out["fdt"][r], out["alpha"][r] = 0, cut, state["alpha0"]
                out["coef"][r] = 0.0, 0.0, cut, 1.0
                branch = "negative"
            if bounds is not None:
                terms = 3 * n
                bounds["E"][r] = nb * EPS * float(np.abs(state["parts"][part][r].astype(LD)).sum() + abs(LD(e)))
                bounds["fmax"][r] = 2 * EPS * float(fm)  # (3 - 1) 2^-52 M on the square, halved by the root, and the root's own rounding
                bounds["b"][r] = float(b) * (terms - 1 + 3) * EPS  # both sums are of positive terms: (terms - 1) 2^-52 relative each,
                # halved by the root; the division, the root and the product round once more each
        if bounds is not None:
            bounds["branch"][r] = branch
    return out


def front(state, part, capped=None):
    """agbnp_md_fire_front: the move the back half decided, then the tethers; partials into parts[part].  `capped`, a list,
    receives per replica the mask of the atoms whose move was scaled to max_move (None where the replica did not move)."""
    out = copy_state(state)
    R = len(state["x"])
    m = state["mass"].astype(LD)[:, None]
    for r in range(R):
        a, b, dt, move = (LD(c) for c in state["coef"][r])
        mask = None
        if move != 0:
            F, W = state["f"][r].astype(LD), state["w"][r].astype(LD)
            W = a * W + b * F
            W = W + (dt / m) * F
            D = dt * W
            length = np.sqrt((D * D).sum(axis=1))
            mask = length > LD(state["max_move"])
            c = np.where(mask, LD(state["max_move"]) / np.where(mask, length, LD(1)), LD(1))[:, None]
            D, W = D * c, W * c
            out["w"][r] = W.astype(np.float64)
            out["x"][r] = (state["x"][r].astype(LD) + D).astype(np.float64)
        if capped is not None:
            capped.append(mask)
        mr._tether_terms(out, r, part)
    return out


# ---- the state's minimiser words ---------------------------------------------------------------------------------------------------

CONSTANTS = dict(f_inc=1.1, f_dec=0.5, alpha0=0.1, f_alpha=0.99, n_min=5)  # (md.FIRE_*: Bitzek et al.)


def add_fire_words(state, dt0, dt_max, tolerance, max_move, capacity, guard=0, fill=0.0):
    """The minimiser's words as minimise() starts them: zeros, dt0 and alpha0; logs (and their guards) full of `fill`."""
    R, n = state["x"].shape[:2]
    state.update(w=np.zeros((R, n, 3)), fdt=np.full(R, float(dt0)), alpha=np.full(R, CONSTANTS["alpha0"]), fmax=np.zeros(R),
                 npos=np.zeros(R, dtype=np.int32), converged=np.zeros(R, dtype=np.int32), voids=np.zeros(R, dtype=np.int32),
                 iterations=np.zeros(R, dtype=np.int64), arrived=np.zeros(R, dtype=np.uint32), coef=np.zeros((R, 4)),
                 fpart=np.zeros((R, blocks(n), 4)), log_e=np.full(R * capacity + 2 * guard, fill), log_fmax=np.full(R * capacity + 2 * guard, fill),
                 fcap=int(capacity), fguard=int(guard), dt_max=float(dt_max), tolerance=float(tolerance), max_move=float(max_move), **CONSTANTS)
    return state


# ---- the synthetic inputs of the kernel tests ------------------------------------------------------------------------------------

ITERATIONS = 16                              # launches pairs per sequence: the n_min branch and the dt_max clamp are met
ITERATION_WORDS = (0, 10, (1 << 32) + 3)     # replicas 0, 1, 2 against logs of FCAP slots; the others start at 0
FCAP, FGUARD = 16, 5
DT0, DT_MAX, TOLERANCE, MAX_MOVE = 0.003, 0.003, 2.0, 1.0e-3
VOID_AT = 4                                  # the iteration whose evaluation is withheld for replica 0
NAN_C = np.uint64(0x7FF8DEADBEEF0003).view(np.float64)
NAN_D = np.uint64(0x7FF8DEADBEEF0004).view(np.float64)


def standin_minimum(state, y0):
    """Where tethers + the harmonic stand-in have their minimum."""
    return (state["k"] * state["x0"] + mr.K2 * y0) / (state["k"] + mr.K2)


def synthetic_state(n, R):
    """md_restatement's synthetic state (sentinels in everything the minimiser must not touch) with the minimiser's words:
    velocities w of either sign of F.w, the iteration words of ITERATION_WORDS, sentinels in coef, fpart, fmax and the logs.
    The LAST replica of R >= 2 starts close to the minimum of tethers + stand-in and nearly at rest: it converges within the sequence
    while the others go on."""
    state = mr.synthetic_state(n, R)
    y0 = mr.standin_anchor(state)
    add_fire_words(state, DT0, DT_MAX, TOLERANCE, MAX_MOVE, FCAP, FGUARD, NAN_C)
    rng = np.random.default_rng(7000 + n)
    state["w"] = rng.normal(0.0, 0.02, (R, n, 3))
    state["iterations"][:min(R, 3)] = ITERATION_WORDS[:R]
    state["log_fmax"][:] = NAN_D
    state["coef"][:], state["fpart"][:], state["fmax"][:] = NAN_C, NAN_D, NAN_C
    state["coef"][:, 3] = 0.0
    if R >= 2:
        near = standin_minimum(state, y0)
        state["x"][R - 1] = near + 1.0e-4 * np.sin(41.0 * near)
        state["w"][R - 1] *= 0.01
    return state, y0


# ---- the same FIRE as a CPU minimiser around any evaluation ----------------------------------------------------------------------

def minimise(evaluate, x, x0, mass, k, tolerance=10.0, max_iterations=1000, dt0=0.001, dt_max=0.005, max_move=0.01):
    """What `_Replicas.minimise` enqueues, for one replica on the CPU: tethers and `evaluate(x[n][3]) -> (energy, forces)`, then
    back, front, evaluation per iteration until the back half reports convergence.  Returns a dict: x (final positions),
    iterations, converged, energy and fmax of the last judged evaluation, the logs, and `capped`, the number of iterations in
    which the move of some atom was scaled to max_move."""
    n = len(x)
    state = dict(x=np.array(x, dtype=np.float64)[None].copy(), f=np.zeros((1, n, 3)), x0=np.array(x0, dtype=np.float64),
                 mass=np.array(mass, dtype=np.float64), k=float(k), energy=np.zeros(1),
                 parts=[np.zeros((1, blocks(n))), np.zeros((1, blocks(n)))])
    add_fire_words(state, dt0, dt_max, tolerance, max_move, max_iterations)

    def evaluated(s):
        e, F = evaluate(s["x"][0])
        s["f"][0] += F
        s["energy"][0] = e
        return s

    state = evaluated(mr.tethers(state, 0))
    capped = 0
    for _ in range(max_iterations):
        state = back(state, 0)
        if state["converged"][0]:
            break
        masks = []
        state = evaluated(front(state, 0, masks))
        capped += int(masks[0] is not None and masks[0].any())
    it = int(state["iterations"][0])
    return dict(x=state["x"][0], iterations=it, converged=bool(state["converged"][0]), energy=float(state["log_e"][it - 1]),
                fmax=float(state["fmax"][0]), log_e=state["log_e"][:it].copy(), log_fmax=state["log_fmax"][:it].copy(), capped=capped)
