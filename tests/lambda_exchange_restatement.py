"""A CPU restatement of agbnp_md_lambda_exchange (openmm_agbnp_plugin_amd/csrc/md_kernels.hip: k_md_lambda_exchange), written
from that file's header comment and DESIGN.md s.4o in numpy.longdouble in the style of tests/hremd_restatement.py, and the
synthetic inputs the tests of the launch share.  A plain module: tests/test_lambda_exchange_api.py checks it against itself on
the CPU, tests/test_gpu_lambda_exchange_kernel.py judges the kernel by it.

The state is a dict holding every word the launch may read or write, each array with a tail of TAIL words no kernel may touch:

  replicas (R, an int)
  lambda, u, kT [R + TAIL] (float64);  step [R + TAIL] (int64)
  rung_of_replica, replica_at_rung [R + TAIL] (int32);  attempts [1 + TAIL] (int64)
  records (md.LAMBDA_RECORD), record_base (the log place of records[0]), log_capacity (a log place, as the kernel's)

`exchange` takes a state and returns the predicted state after the launch -- the words that must not change included -- and
leaves its argument alone.  Delta and the verdict are formed in long double from the doubles the kernel reads; everything the
kernel stores is a copy of a word it read, an integer or a zero.  All R u words come back as zeros, those of the replicas that sat
the attempt out too (the driver's next attempt adds to all of them again)."""
import numpy as np

from openmm_agbnp_plugin_amd import md
from tests import md_restatement as mr

LD = np.longdouble
_M32, _M64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF
TAIL = 2
LAMBDA_WORD, TEMPERATURE_WORD = 4, 2  # the Philox counter's fourth word: this exchange's, and md_restatement.exchange's
INT_SENTINEL = 0x7EADBEEF


def pairs(a, R):
    """The rung pairs (k, k + 1) of attempt a, in the order of the kernel's threads."""
    return [(k, k + 1) for k in range(a & 1, R - 1, 2)]


def delta_of(lambda_lo, lambda_hi, kT_lo, kT_hi, u_lo, u_hi):
    """Delta in long double from doubles (md.lambda_delta's expression)."""
    l_lo, l_hi, kT_lo, kT_hi, u_lo, u_hi = (LD(w) for w in (lambda_lo, lambda_hi, kT_lo, kT_hi, u_lo, u_hi))
    return (l_lo - l_hi) * (u_lo / kT_lo - u_hi / kT_hi)


def is_void(u_lo, u_hi):
    return bool(u_lo == 0.0 or u_hi == 0.0 or not np.isfinite(u_lo) or not np.isfinite(u_hi))


def exchange(state, seed, counter_word=LAMBDA_WORD):
    """agbnp_md_lambda_exchange: one attempt between neighbouring rungs.  `counter_word`: the fourth word of the Philox counter
    (4; 2 gives the deviates of the temperature exchange)."""
    out = mr.copy_state(state)
    R, a, seed = int(out["replicas"]), int(out["attempts"][0]), int(seed) & _M64
    first = mr.exchange_places(a, R)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for t, (k, k1) in enumerate(pairs(a, R)):
            lo, hi = int(state["replica_at_rung"][k]), int(state["replica_at_rung"][k1])
            l_lo, l_hi = state["lambda"][lo], state["lambda"][hi]
            kT_lo, kT_hi, u_lo, u_hi = state["kT"][lo], state["kT"][hi], state["u"][lo], state["u"][hi]
            w = md.philox4x32((k, a & _M32, (a >> 32) & _M32, counter_word), (seed & _M32, seed >> 32))
            uniform = md.uniform53(w[0], w[1])
            void = is_void(u_lo, u_hi)
            accepted = not void and bool(np.log(LD(uniform)) <= delta_of(l_lo, l_hi, kT_lo, kT_hi, u_lo, u_hi))
            if accepted:
                out["lambda"][lo], out["lambda"][hi] = l_hi, l_lo
                out["rung_of_replica"][lo], out["rung_of_replica"][hi] = k1, k
                out["replica_at_rung"][k], out["replica_at_rung"][k1] = hi, lo
            at = first + t
            if at < int(out["log_capacity"]):
                place = at - int(out["record_base"])
                if not 0 <= place < len(out["records"]):
                    raise IndexError(f"record place {at} lies outside the buffer")
                out["records"][place] = (a, int(state["step"][lo]), k, lo, hi, -1 if void else int(accepted), u_lo, u_hi, l_lo, l_hi,
                                         kT_lo, kT_hi, uniform)
    out["u"][:R] = 0.0  # all R words, read or not; the tail stays
    out["attempts"][0] = a + 1
    return out


# ---- the synthetic inputs of the tests -------------------------------------------------------------------------------------------

EXCHANGE_SEED = mr.EXCHANGE_SEED
FIRST_ATTEMPT = mr.FIRST_ATTEMPT  # 2^32 - 3: both parities and the carry into the counter's high word within four attempts
ATTEMPTS = 16
ENERGY_SEED = 411  # (chosen once on the CPU: tests/test_lambda_exchange_api.py shows that with it no verdict lies in the band)
SIZES = (1, 2, 3, 8, 16)
BAND = 1e-9  # a verdict is compared where |log(uniform) - Delta| > BAND max(1, |Delta|)


def ladder(R):
    """The lambda of rung k: even from 0 to 1 (a single rung: 0.5)."""
    return np.linspace(0.0, 1.0, R) if R > 1 else np.array([0.5])


def _tailed(values, sentinel, dtype=np.float64):
    return np.concatenate([np.asarray(values, dtype=dtype), np.full(TAIL, sentinel, dtype=dtype)])


def lambda_state(R, log_capacity=None, buffer=None, first_attempt=FIRST_ATTEMPT, attempts=ATTEMPTS):
    """The launch's words in front of the first attempt: replica r on rung r with the ladder's lambda_r, a bath of its own
    (KB 300 1.02^r), step[r] = 1000 + 7 r, the attempt counter at 2^32 - 3, the u words and every tail full of sentinels.  The
    record buffer starts at the log place of the first attempt's first record (`record_base`) and is full of 0xFF; `log_capacity`
    (in records of this run, default: all of them) becomes the log place the kernel compares with.  `energies` fills in what an
    attempt reads."""
    base = mr.exchange_places(first_attempt, R)
    total = mr.exchange_places(first_attempt + attempts, R) - base
    buffer = max(total, 1) if buffer is None else buffer
    records = np.frombuffer(bytes([0xFF]) * (buffer * md.LAMBDA_RECORD.itemsize), dtype=md.LAMBDA_RECORD).copy()
    state = dict(replicas=R, kT=_tailed(md.KB * 300.0 * 1.02 ** np.arange(R), mr.NAN_B), u=np.full(R + TAIL, mr.NAN_A),
                 step=_tailed(1000 + 7 * np.arange(R), -77, np.int64),
                 rung_of_replica=_tailed(np.arange(R), INT_SENTINEL, np.int32), replica_at_rung=_tailed(np.arange(R), INT_SENTINEL, np.int32),
                 attempts=_tailed([first_attempt], -99, np.int64), records=records, record_base=base,
                 log_capacity=base + (total if log_capacity is None else log_capacity))
    state["lambda"] = _tailed(ladder(R), mr.NAN_A)
    return state


def energies(state, i):
    """The state in front of attempt number i of a run (a copy): the u words of the replicas on the attempt's pairs from a
    generator seeded by (ENERGY_SEED, R, i) -- binding energies around 440 kJ/mol, 40 wide, so that |Delta| reaches a few units
    at R = 2 and some tenths at R = 16 and both verdicts occur --, sentinels in the u words of the replicas that sit it out."""
    out = mr.copy_state(state)
    R, a = int(out["replicas"]), int(out["attempts"][0])
    rng = np.random.default_rng([ENERGY_SEED, R, i])
    u = rng.normal(440.0, 40.0, R)
    out["u"][:] = mr.NAN_A
    for pair in pairs(a, R):
        for k in pair:
            r = int(out["replica_at_rung"][k])
            out["u"][r] = u[r]
    return out


CRAFTED = ("accept", "reject", "void0", "voidneg0", "voidnan", "voidinf")  # the pairs (0,1), (2,3), ... of an even attempt


def set_pair(state, k, kind):
    """Overwrites what the pair of rungs (k, k + 1) of `state` reads.  "accept": Delta = +50 whatever the deviate is
    (log(uniform) >= -36.8);  "reject": Delta = -50;  "void0" / "voidneg0": u_lo = 0.0 / -0.0;  "voidnan" / "voidinf": u_hi = NaN /
    -inf."""
    lo, hi = int(state["replica_at_rung"][k]), int(state["replica_at_rung"][k + 1])
    if kind in ("accept", "reject"):
        sign = 1.0 if kind == "accept" else -1.0
        d = state["lambda"][lo] - state["lambda"][hi]
        state["u"][hi] = 400.0
        state["u"][lo] = state["kT"][lo] * (400.0 / state["kT"][hi] + sign * 50.0 / d)
    elif kind == "void0":
        state["u"][lo] = 0.0
    elif kind == "voidneg0":
        state["u"][lo] = -0.0
    elif kind == "voidnan":
        state["u"][hi] = np.nan
    elif kind == "voidinf":
        state["u"][hi] = -np.inf
    else:
        raise ValueError(kind)
    return state


def crafted_state(R=16):
    """R = 16 in front of an EVEN attempt (2^32 - 2) whose first six pairs are the certain cases of `set_pair`."""
    state = energies(lambda_state(R, first_attempt=FIRST_ATTEMPT + 1, attempts=1), 0)
    for j, kind in enumerate(CRAFTED):
        set_pair(state, 2 * j, kind)
    return state


def margin(rec):
    """(|log(uniform) - Delta| / max(1, |Delta|), Delta) of a record, in long double."""
    d = delta_of(rec["lambda_lo"], rec["lambda_hi"], rec["kT_lo"], rec["kT_hi"], rec["u_lo"], rec["u_hi"])
    return float(abs(np.log(LD(rec["uniform"])) - d) / max(LD(1), abs(d))), d
