"""A CPU restatement of agbnp_md_hamiltonian_exchange (openmm_agbnp_plugin_amd/csrc/md_kernels.hip: k_md_hamiltonian_decide, then
k_md_hamiltonian_apply), written from that file's header comment and DESIGN.md s.4k in numpy.longdouble in the style of
tests/md_restatement.py::exchange, and the synthetic inputs the tests of the two kernels share.  A plain module:
tests/test_hremd_api.py checks it against itself and against md_restatement.exchange on the CPU, tests/test_gpu_hremd_kernels.py
judges the kernels by it.

The state is a dict of numpy arrays holding every word the kernels may read or write:

  x, v, f [R][n][3];  kT [R];  last [R][2];  step [R] (int64);  parts: the two tether-partial buffers, [R][blocks(n)] each
  cross, scale [R + TAIL] (float64) and partner [R + TAIL] (int32): the words of the R slots and a tail no kernel may touch
  walker_at_rung, rung_of_walker [R] (int32);  attempts [1] (int64)
  records (md.HAMILTONIAN_RECORD), record_base (the log place of records[0]), log_capacity (a log place, as the kernel's)

`exchange` takes a state and returns the predicted state after the two launches -- the words that must not change included --
and leaves its argument alone.  Delta and the verdict are formed in long double from the doubles the kernel reads; what the
kernel stores in a double (the tether sums, the kinetic words, the velocities) is rounded to a double where it is stored.  The
velocity factors are formed in double, as md_restatement.exchange forms them."""
import numpy as np

from openmm_agbnp_plugin_amd import md
from tests import md_restatement as mr

LD = np.longdouble
_M32, _M64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF
TAIL = 2
PARTNER_SENTINEL = 0x7EADBEEF
HAMILTONIAN_WORD, TEMPERATURE_WORD = 3, 2  # the Philox counter's fourth word: this exchange's, and md_restatement.exchange's


def pairs(a, R):
    """The slot pairs (k, k + 1) of attempt a, in the order of the kernel's threads."""
    return [(k, k + 1) for k in range(a & 1, R - 1, 2)]


def delta_of(kT_lo, kT_hi, p_lo, p_hi, t_lo, t_hi, c_lo, c_hi):
    """Delta in long double from doubles (md.hamiltonian_delta's expression)."""
    kT_lo, kT_hi, p_lo, p_hi, t_lo, t_hi, c_lo, c_hi = (LD(w) for w in (kT_lo, kT_hi, p_lo, p_hi, t_lo, t_hi, c_lo, c_hi))
    return ((p_lo - t_lo) - c_lo) / kT_lo + ((p_hi - t_hi) - c_hi) / kT_hi + (LD(1) / kT_lo - LD(1) / kT_hi) * (t_lo - t_hi)


def is_void(c_lo, c_hi):
    return bool(c_lo == 0.0 or c_hi == 0.0 or not np.isfinite(c_lo) or not np.isfinite(c_hi))


def exchange(state, seed, part, counter_word=HAMILTONIAN_WORD):
    """agbnp_md_hamiltonian_exchange: one attempt between neighbouring slots (decide, then exchange the conformations); the tether
    partials read are parts[part].  `counter_word`: the fourth word of the Philox counter (3; 2 gives the deviates of the
    temperature exchange, for the comparison with md_restatement.exchange)."""
    out = mr.copy_state(state)
    R, a, seed = len(out["kT"]), int(out["attempts"][0]), int(seed) & _M64
    out["partner"][:R], out["scale"][:R] = -1, 1.0
    first = mr.exchange_places(a, R)
    with np.errstate(invalid="ignore", over="ignore"):
        for t, (lo, hi) in enumerate(pairs(a, R)):
            kT_lo, kT_hi = state["kT"][lo], state["kT"][hi]
            p_lo, p_hi, k_lo, k_hi = state["last"][lo, 0], state["last"][hi, 0], state["last"][lo, 1], state["last"][hi, 1]
            t_lo, t_hi = (np.float64(state["parts"][part][r].astype(LD).sum()) for r in (lo, hi))
            c_lo, c_hi = state["cross"][lo], state["cross"][hi]
            out["cross"][lo] = out["cross"][hi] = 0.0
            w_lo, w_hi = int(state["walker_at_rung"][lo]), int(state["walker_at_rung"][hi])
            w = md.philox4x32((lo, a & _M32, (a >> 32) & _M32, counter_word), (seed & _M32, seed >> 32))
            u = md.uniform53(w[0], w[1])
            void = is_void(c_lo, c_hi)
            accepted = not void and bool(np.log(LD(u)) <= delta_of(kT_lo, kT_hi, p_lo, p_hi, t_lo, t_hi, c_lo, c_hi))
            if accepted:
                out["partner"][lo], out["partner"][hi] = hi, lo
                out["scale"][lo], out["scale"][hi] = np.sqrt(kT_lo / kT_hi), np.sqrt(kT_hi / kT_lo)
                out["walker_at_rung"][lo], out["walker_at_rung"][hi] = w_hi, w_lo
                out["rung_of_walker"][w_lo], out["rung_of_walker"][w_hi] = hi, lo
                out["last"][lo, 1] = np.float64(LD(k_hi) * LD(kT_lo) / LD(kT_hi))
                out["last"][hi, 1] = np.float64(LD(k_lo) * LD(kT_hi) / LD(kT_lo))
            at = first + t
            if at < int(out["log_capacity"]):
                place = at - int(out["record_base"])
                if not 0 <= place < len(out["records"]):
                    raise IndexError(f"record place {at} lies outside the buffer")
                out["records"][place] = (a, int(state["step"][lo]), lo, w_lo, w_hi, -1 if void else int(accepted), p_lo, p_hi, t_lo, t_hi,
                                         c_lo, c_hi, kT_lo, kT_hi, u)
    out["attempts"][0] = a + 1
    for r in range(R):
        q = int(out["partner"][r])
        if q > r:
            out["x"][r], out["x"][q] = state["x"][q].copy(), state["x"][r].copy()
            out["v"][r], out["v"][q] = state["v"][q] * out["scale"][r], state["v"][r] * out["scale"][q]
    return out


# ---- the synthetic inputs of the tests -------------------------------------------------------------------------------------------

EXCHANGE_SEED = mr.EXCHANGE_SEED
FIRST_ATTEMPT = mr.FIRST_ATTEMPT  # 2^32 - 3: both parities and the carry into the counter's high word within four attempts
ATTEMPTS = 16
ENERGY_SEED = 302  # (chosen once on the CPU: tests/test_hremd_api.py shows that with it no verdict hangs on the last bits)


def hamiltonian_state(n, R, log_capacity=None, buffer=None, first_attempt=FIRST_ATTEMPT, attempts=ATTEMPTS, ratio=1.05):
    """The kernels' words in front of the first attempt: the ladder KB 300 ratio^k, walker w on rung w, step[k] = 1000 + 7 k, the
    attempt counter at 2^32 - 3, partner / scale / cross tails and both partial buffers full of sentinels.  The record buffer
    starts at the log place of the first attempt's first record (`record_base`) and is full of 0xFF; `log_capacity` (in records
    of this run, default: all of them) becomes the log place the kernel compares with.  `energies` fills in what an attempt reads."""
    rng = np.random.default_rng(2000 + 17 * n + R)
    base = mr.exchange_places(first_attempt, R)
    total = mr.exchange_places(first_attempt + attempts, R) - base
    buffer = max(total, 1) if buffer is None else buffer
    records = np.frombuffer(bytes([0xFF]) * (buffer * md.HAMILTONIAN_RECORD.itemsize), dtype=md.HAMILTONIAN_RECORD).copy()
    return dict(x=rng.uniform(0.0, 4.0, (R, n, 3)), v=rng.normal(size=(R, n, 3)), f=rng.normal(0.0, 500.0, (R, n, 3)),
                kT=md.KB * 300.0 * ratio ** np.arange(R), last=np.full((R, 2), mr.NAN_B), step=1000 + 7 * np.arange(R, dtype=np.int64),
                parts=[np.full((R, mr.blocks(n)), mr.NAN_A), np.full((R, mr.blocks(n)), mr.NAN_B)],
                cross=np.full(R + TAIL, mr.NAN_A), scale=np.full(R + TAIL, mr.NAN_B), partner=np.full(R + TAIL, PARTNER_SENTINEL, dtype=np.int32),
                walker_at_rung=np.arange(R, dtype=np.int32), rung_of_walker=np.arange(R, dtype=np.int32),
                attempts=np.array([first_attempt], dtype=np.int64), records=records, record_base=base,
                log_capacity=base + (total if log_capacity is None else log_capacity))


def energies(state, i, part, one_hamiltonian=False):
    """The state in front of attempt number i of a run (a copy): fresh positions and velocities, the slots that sit the attempt
    out holding sentinels in both; last = {P, K}, the tether partials of parts[part] (the other buffer all sentinels) and the
    cross words of the attempt's pairs (sentinels elsewhere) from a generator seeded by (ENERGY_SEED, R, i).  Conformation j has an energy
    e_j around -1000 kJ/mol, 30 wide; slot k sees it as A_k(x_j) = s_k e_j with s_k = 1 - 0.002 k (all 1 for `one_hamiltonian`:
    the cross words are then the partner's own AGBNP energy bit for bit) plus, for the cross words, noise of 1 kJ/mol."""
    out = mr.copy_state(state)
    R, n = out["x"].shape[:2]
    a = int(out["attempts"][0])
    rng = np.random.default_rng([ENERGY_SEED, R, i])
    out["x"], out["v"] = rng.uniform(0.0, 4.0, (R, n, 3)), rng.normal(size=(R, n, 3))
    s = np.ones(R) if one_hamiltonian else 1.0 - 0.002 * np.arange(R)
    e = rng.normal(-1000.0, 30.0, R)
    out["parts"] = [np.full((R, mr.blocks(n)), mr.NAN_A), np.full((R, mr.blocks(n)), mr.NAN_B)]
    out["parts"][part] = rng.uniform(50.0, 200.0, (R, mr.blocks(n)))
    tether = out["parts"][part].astype(LD).sum(axis=1).astype(np.float64)
    own = s * e
    out["last"] = np.stack([own + tether, rng.uniform(800.0, 1000.0, R)], axis=1)
    out["cross"][:] = mr.NAN_A
    busy = set()
    for lo, hi in pairs(a, R):
        busy.update((lo, hi))
        if one_hamiltonian:  # what the kernel forms as P - T of the partner, so that the pair's Delta is exchange_delta's
            out["cross"][lo], out["cross"][hi] = out["last"][hi, 0] - tether[hi], out["last"][lo, 0] - tether[lo]
        else:
            out["cross"][lo], out["cross"][hi] = s[lo] * e[hi] + rng.normal(), s[hi] * e[lo] + rng.normal()
    for r in set(range(R)) - busy:
        out["x"][r], out["v"][r] = mr.NAN_A, mr.NAN_B
    return out


def set_pair(state, part, lo, kind):
    """Overwrites what the pair (lo, lo + 1) of `state` reads.  "accept": Delta = +400 whatever u is (log u >= -36.8);  "reject":
    Delta = -400;  "equal": equal baths, energies, tethers and cross words equal to P - T: Delta is exactly 0, accepted, both
    factors exactly 1;  "void0": C_lo left 0.0;  "voidinf": C_hi = inf."""
    hi = lo + 1
    t = [np.float64(state["parts"][part][r].astype(LD).sum()) for r in (lo, hi)]
    if kind in ("accept", "reject"):
        sign = 1.0 if kind == "accept" else -1.0
        state["parts"][part][hi] = state["parts"][part][lo]  # (T_lo == T_hi: the tether term vanishes)
        state["cross"][lo] = (state["last"][lo, 0] - t[0]) - sign * 400.0 * state["kT"][lo]
        state["cross"][hi] = state["last"][hi, 0] - t[0]
    elif kind == "equal":
        state["kT"][hi] = state["kT"][lo]
        state["parts"][part][hi] = state["parts"][part][lo]
        state["last"][hi, 0] = state["last"][lo, 0]
        state["cross"][lo] = state["cross"][hi] = state["last"][lo, 0] - t[0]
    elif kind == "void0":
        state["cross"][lo] = 0.0
    elif kind == "voidinf":
        state["cross"][hi] = np.inf
    else:
        raise ValueError(kind)
    return state


def margin(rec):
    """|log u - Delta| / max(1, |Delta|) of a record, in long double: a verdict is judged where this is at least 1e-12."""
    d = delta_of(rec["kT_lo"], rec["kT_hi"], rec["P_lo"], rec["P_hi"], rec["T_lo"], rec["T_hi"], rec["C_lo"], rec["C_hi"])
    return float(abs(np.log(LD(rec["u"])) - d) / max(LD(1), abs(d))), d
