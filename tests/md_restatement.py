"""A CPU restatement of every entry point of libagbnp_md.so (openmm_agbnp_plugin_amd/csrc/md_kernels.hip), written from that
file's header comment and DESIGN.md s.4j in numpy.longdouble, and the synthetic inputs the tests of the kernels share.  A plain
module: tests/test_md_restatement.py checks it against itself on the CPU, tests/test_gpu_md_kernels.py judges the kernels by it.

The state is a dict of numpy arrays holding every word the kernels may read or write:

  x, v, f [R][n][3];  x0 [n][3];  hdt_m, mass [n];  kT [R];  seeds [R] (uint64);  c1, dt, k (floats)
  energy [R];  acc [R][2];  done [R] (uint32);  step [R] (int64);  last [R][2]
  log_pe, log_ke: flat, [R][capacity] followed by a padding tail no kernel may touch;  capacity
  parts: the two tether-partial buffers, [R][blocks(n)] each
  and for the exchange: rung_of_replica, replica_at_rung [R] (int32);  attempts [1] (int64);  scale [R];
  records (md.EXCHANGE_RECORD), record_base (the log place of records[0]), log_capacity (a log place, as the kernel's)

Every function takes a state and returns the predicted state after ONE launch -- the words that must not change included --
and leaves its argument alone.  What a kernel keeps in a double is rounded to a double here where it is stored and where the
next operation reads it (a stored position before the tether term, the velocity at the end of a step before the next first
kick); everything between two such words is long double.  Where long double is wider than double this is a higher-precision
reference; where it is not, it is the same arithmetic without the kernels' contraction and summation order.  The exchange's
velocity factors are formed in double: an IEEE division and square root, correctly rounded on both sides, so they are expected
bit for bit.  Philox and the 53-bit uniforms are the module's own (md.philox4x32 / md.uniform53, pinned to the Random123 known
answers by tests/test_replica_md_api.py)."""
import numpy as np

from openmm_agbnp_plugin_amd import md

LD = np.longdouble
BLOCK = 256  # threads, and atoms, of one workgroup
LANGEVIN, VERLET = 0, 1
_M32, _M64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF
TWO_PI = LD(8) * np.arctan(LD(1))


def blocks(n):
    return (n + BLOCK - 1) // BLOCK


def copy_state(state):
    out = {}
    for key, val in state.items():
        out[key] = [p.copy() for p in val] if key == "parts" else (val.copy() if isinstance(val, np.ndarray) else val)
    return out


def deviates(n, seed, s):
    """Three standard normal deviates per atom: Philox blocks a, b with counter (atom, s lo, s hi, 0 | 1) and key seed, Box-Muller
    on the 53-bit uniforms, z = (ra cos, ra sin, rb cos) with the phase 2 pi u."""
    seed, s = int(seed) & _M64, int(s) & _M64
    key, lo, hi = (seed & _M32, seed >> 32), s & _M32, s >> 32
    u = np.empty((n, 4))
    for i in range(n):
        a, b = md.philox4x32((i, lo, hi, 0), key), md.philox4x32((i, lo, hi, 1), key)
        u[i] = md.uniform53(a[0], a[1]), md.uniform53(a[2], a[3]), md.uniform53(b[0], b[1]), md.uniform53(b[2], b[3])
    u = u.astype(LD)
    ra, rb = np.sqrt(LD(-2) * np.log(u[:, 0])), np.sqrt(LD(-2) * np.log(u[:, 2]))
    pa, pb = TWO_PI * u[:, 1], TWO_PI * u[:, 3]
    return np.stack([ra * np.cos(pa), ra * np.sin(pa), rb * np.cos(pb)], axis=1)


def _block_sums(per_atom):
    n = len(per_atom)
    return np.array([per_atom[b * BLOCK:(b + 1) * BLOCK].sum() for b in range(blocks(n))], dtype=LD).astype(np.float64)


def _tether_terms(out, r, part):
    """f = -k (x - x0) at the stored positions of replica r, the tethers' energy as per-block partials."""
    dd = out["x"][r].astype(LD) - out["x0"].astype(LD)
    k = LD(out["k"])
    out["f"][r] = (-k * dd).astype(np.float64)
    out["parts"][part][r] = _block_sums((LD(0.5) * k * dd * dd).sum(axis=1))


def _front(out, r, kind, pv, s, part):
    """The front half of step s of replica r, velocity pv (long double) already kicked: drift (+ OU at kT[r]), tethers."""
    x, m = out["x"][r].astype(LD), out["mass"].astype(LD)[:, None]
    dt, c1 = LD(out["dt"]), LD(out["c1"])
    if kind == LANGEVIN:
        z = deviates(len(x), out["seeds"][r], s)
        cn = np.sqrt((LD(1) - c1 * c1) * LD(out["kT"][r]) / m)
        px = x + LD(0.5) * dt * pv
        pv = c1 * pv + cn * z
        px = px + LD(0.5) * dt * pv
    elif kind == VERLET:
        px = x + dt * pv
    else:
        raise ValueError(f"kind {kind}")
    out["x"][r], out["v"][r] = px.astype(np.float64), pv.astype(np.float64)
    _tether_terms(out, r, part)


def _second_kick(out, r):
    """v += dt/2m f, stored; returns the kinetic energy of the stored velocities."""
    h, m = out["hdt_m"].astype(LD)[:, None], out["mass"].astype(LD)[:, None]
    out["v"][r] = (out["v"][r].astype(LD) + h * out["f"][r].astype(LD)).astype(np.float64)
    v1 = out["v"][r].astype(LD)
    return (LD(0.5) * m * v1 * v1).sum()


def _log_step(out, r, kin, part):
    """What the replica's last workgroup to arrive does: potential = tether partials + the energy word, both energies into the
    logs at the step word (if the logs reach that far) and into `last`; step + 1; energy, acc[r][0], done handed back as zeros."""
    s, cap = int(out["step"][r]), int(out["capacity"])
    pot = np.float64(out["parts"][part][r].astype(LD).sum() + LD(out["energy"][r]))
    kin = np.float64(LD(out["acc"][r, 0]) + kin)
    if s < cap:
        out["log_pe"][r * cap + s], out["log_ke"][r * cap + s] = pot, kin
    out["last"][r] = pot, kin
    out["step"][r] = s + 1
    out["energy"][r], out["acc"][r, 0], out["done"][r] = 0.0, 0.0, 0


def tethers(state, part):
    """agbnp_md_group_tethers: the tethers alone, partials into parts[part]."""
    out = copy_state(state)
    for r in range(len(out["x"])):
        _tether_terms(out, r, part)
    return out


def pre(state, kind, part):
    """agbnp_md_group_pre: everything in front of the force evaluation of step step[r]; partials into parts[part]."""
    out = copy_state(state)
    h = out["hdt_m"].astype(LD)[:, None]
    for r in range(len(out["x"])):
        pv = out["v"][r].astype(LD) + h * out["f"][r].astype(LD)
        _front(out, r, kind, pv, int(out["step"][r]), part)
    return out


def post(state, part):
    """agbnp_md_group_post: everything behind it; the tether partials read are parts[part]."""
    out = copy_state(state)
    for r in range(len(out["x"])):
        _log_step(out, r, _second_kick(out, r), part)
    return out


def mid(state, kind, part_old, part_new=None):
    """agbnp_md_group_mid: the back half of step s (partials read: parts[part_old]) and the front half of step s + 1 (partials
    written: parts[part_new], the other buffer unless given) in one launch: the same force kicks twice."""
    part_new = 1 - part_old if part_new is None else part_new
    out = copy_state(state)
    h = out["hdt_m"].astype(LD)[:, None]
    for r in range(len(out["x"])):
        s = int(out["step"][r])
        kin = _second_kick(out, r)                                      # the end of step s
        pv = out["v"][r].astype(LD) + h * out["f"][r].astype(LD)        # the first kick of step s + 1
        _front(out, r, kind, pv, s + 1, part_new)
        _log_step(out, r, kin, part_old)
    return out


def exchange_places(a, R):
    """The log place of the first record of attempt a: attempts 0 .. a - 1 left (a + 1) / 2 even ones with R / 2 pairs each and
    a / 2 odd ones with (R - 1) / 2."""
    return ((a + 1) // 2) * (R // 2) + (a // 2) * ((R - 1) // 2)


def exchange(state, seed):
    """agbnp_md_exchange: one attempt between neighbouring rungs (decide, then rescale)."""
    out = copy_state(state)
    R, a, seed = len(out["kT"]), int(out["attempts"][0]), int(seed) & _M64
    out["scale"][:] = 1.0
    first = exchange_places(a, R)
    for t, k in enumerate(range(a & 1, R - 1, 2)):
        lo, hi = int(state["replica_at_rung"][k]), int(state["replica_at_rung"][k + 1])
        kT_lo, kT_hi = state["kT"][lo], state["kT"][hi]
        u_lo, u_hi = state["last"][lo, 0], state["last"][hi, 0]
        delta = (LD(1) / LD(kT_lo) - LD(1) / LD(kT_hi)) * (LD(u_lo) - LD(u_hi))
        w = md.philox4x32((k, a & _M32, (a >> 32) & _M32, 2), (seed & _M32, seed >> 32))
        u = md.uniform53(w[0], w[1])
        accepted = bool(np.log(LD(u)) <= delta)
        if accepted:
            out["kT"][lo], out["kT"][hi] = kT_hi, kT_lo
            out["rung_of_replica"][lo], out["rung_of_replica"][hi] = k + 1, k
            out["replica_at_rung"][k], out["replica_at_rung"][k + 1] = hi, lo
            out["scale"][lo], out["scale"][hi] = np.sqrt(kT_hi / kT_lo), np.sqrt(kT_lo / kT_hi)
        at = first + t
        if at < int(out["log_capacity"]):
            place = at - int(out["record_base"])
            if not 0 <= place < len(out["records"]):
                raise IndexError(f"record place {at} lies outside the buffer")
            out["records"][place] = (a, int(state["step"][lo]), k, lo, hi, int(accepted), u_lo, u_hi, kT_lo, kT_hi, u)
    out["attempts"][0] = a + 1
    for r in range(R):
        if out["scale"][r] != 1.0:
            out["v"][r] = out["v"][r] * out["scale"][r]
    return out


# ---- the synthetic inputs of the tests -------------------------------------------------------------------------------------------

NAN_A = np.uint64(0x7FF8DEADBEEF0001).view(np.float64)  # sentinels: quiet NaNs with a payload, compared as bits
NAN_B = np.uint64(0x7FF8DEADBEEF0002).view(np.float64)
ACC1 = -7.25e300                                        # acc[r][1], which no kernel touches
K2 = 500.0                                              # the stand-in evaluation's spring, kJ/mol/nm^2
START_STEPS = (5, 7, (1 << 32) + 3)                     # replicas 0, 1, 2; the others start at 0
EXCHANGE_SEED = 0x1234567890ABCDEF
FIRST_ATTEMPT = (1 << 32) - 3


def seed_word(r):
    return (0x9E3779B97F4A7C15 * (r + 1) + 0x1234567890ABCDEF) & _M64


def synthetic_state(n, R, capacity=8, tail=5, steps=START_STEPS, dt=0.001, k=2.0e4, friction=10.0):
    """n atoms in a 4 nm box, hydrogens by a 40 % coin, every replica off the tether minimum and with velocities of its own bath;
    logs, their tail and both partial buffers full of NaN sentinels; acc[r][0] and done zero, the kernels' contract."""
    rng = np.random.default_rng(n)
    x0 = rng.uniform(0.0, 4.0, (n, 3))
    mass = np.where(rng.random(n) < 0.4, 1.008, 12.0)
    kT = md.KB * (280.0 + 20.0 * np.arange(R))
    x = x0[None] + 0.002 * np.sin(37.0 * x0[None] + np.arange(R)[:, None, None])
    v = rng.normal(size=(R, n, 3)) * np.sqrt(kT[:, None, None] / mass[None, :, None])
    f = rng.normal(0.0, 500.0, (R, n, 3))
    step = np.zeros(R, dtype=np.int64)
    step[:min(R, len(steps))] = steps[:R]
    acc = np.zeros((R, 2))
    acc[:, 1] = ACC1
    return dict(x=x, v=v, f=f, x0=x0, hdt_m=0.5 * dt / mass, mass=mass, kT=kT,
                seeds=np.array([seed_word(r) for r in range(R)], dtype=np.uint64), c1=float(np.exp(-friction * dt)), dt=dt, k=k,
                energy=np.zeros(R), acc=acc, done=np.zeros(R, dtype=np.uint32), step=step, last=np.full((R, 2), NAN_B),
                log_pe=np.full(R * capacity + tail, NAN_A), log_ke=np.full(R * capacity + tail, NAN_B), capacity=capacity,
                parts=[np.full((R, blocks(n)), NAN_A), np.full((R, blocks(n)), NAN_B)])


def standin_anchor(state):
    """y0 of the stand-in evaluation: the tether anchors moved by 0.05 nm in every component (standard deviation)."""
    n = len(state["x0"])
    return state["x0"] + 0.05 * np.random.default_rng(n + 1).normal(size=(n, 3))


def standin(x, y0):
    """The stand-in for the AGBNP evaluation in double, as the tests upload it: F = -k2 (x - y0) [R][n][3], E = k2/2 sum (x - y0)^2 [R]."""
    d = x - y0[None]
    return -K2 * d, 0.5 * K2 * (d * d).sum(axis=(1, 2))


def evaluated(state, y0):
    """The state after the stand-in evaluation: f += F, energy = E."""
    out = copy_state(state)
    F, E = standin(out["x"], y0)
    out["f"] = out["f"] + F
    out["energy"] = E
    return out


def exchange_state(n, R, log_capacity=None, buffer=None, first_attempt=FIRST_ATTEMPT, attempts=64):
    """The exchange kernels' words: the ladder KB 300 1.05^k with replica r on rung r, step[r] = 1000 + 7 r, random velocities,
    the attempt counter at 2^32 - 3.  The record buffer starts at the log place of the first attempt's first record
    (`record_base`); `log_capacity` (in records of this run, default: all of them) becomes the log place the kernel compares with."""
    rng = np.random.default_rng(1000 + 17 * n + R)
    base = exchange_places(first_attempt, R)
    total = exchange_places(first_attempt + attempts, R) - base
    buffer = max(total, 1) if buffer is None else buffer
    records = np.frombuffer(bytes([0xFF]) * (buffer * md.EXCHANGE_RECORD.itemsize), dtype=md.EXCHANGE_RECORD).copy()
    return dict(v=rng.normal(size=(R, n, 3)), kT=md.KB * 300.0 * 1.05 ** np.arange(R), rung_of_replica=np.arange(R, dtype=np.int32),
                replica_at_rung=np.arange(R, dtype=np.int32), last=np.full((R, 2), NAN_B), step=1000 + 7 * np.arange(R, dtype=np.int64),
                attempts=np.array([first_attempt], dtype=np.int64), scale=np.full(R, 7.0), records=records, record_base=base,
                log_capacity=base + (total if log_capacity is None else log_capacity))


def exchange_energies(R, attempts=64):
    """last[:, 0] before every attempt: [attempts][R] potential energies around -1000 kJ/mol, 30 wide."""
    rng = np.random.default_rng(100 + R)
    return np.array([rng.normal(-1000.0, 30.0, R) for _ in range(attempts)])
