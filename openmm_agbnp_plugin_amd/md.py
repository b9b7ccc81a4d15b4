"""Device-resident molecular dynamics around the AGBNP engine, for the py3 counterparts of the reference's example
scripts (example/test_agbnp.py: minimise, Langevin equilibration, NVE energy-conservation run; example/1dwc_benchmark.py:
Langevin timing run), for the energy-conservation test and for replica exchange (examples/remd_benchmark.py: temperatures,
examples/hremd_benchmark.py: Hamiltonians).

The reference gets its bonded and Coulomb/LJ terms from OpenMM's OPLS system (DesmondDMSFile.createSystem), which is
outside this repository; here the only force-field term besides AGBNP is a harmonic tether of every atom to its start
position, which keeps the geometry a protein.  Everything lives on the GPU: torch tensors for the integrator state, the
engine's device entry points for the force.

One state core, three drivers.  `_Replicas` holds the state of R >= 1 replicas of one system as strided arrays and makes the
integrator's launches: two of libagbnp_md.so (csrc/md_kernels.hip: everything in front of the force evaluation, everything
behind it -- between the steps of a run both in ONE launch; Philox normal deviates) around an evaluation its driver supplies.
`DeviceMD` is the core at R = 1 around `agbnp_hip_execute_device`, its steps captured ONCE as a HIP graph and replayed; the
host only synchronises every `check_every` steps to read the engine's overflow log (agbnp_hip_finish).  `ReplicaMD` is the
core around `agbnp_hip_execute_group`, eager (group calls are not captured), plus temperature exchanges decided on the
device; `HamiltonianReplicaMD` is the same with contexts that differ in their parameters and conformations that
move between them (s.4k); `BindingReplicaMD` is the core around `agbnp_hip_binding_execute_group`, replicas on a ladder of
binding Hamiltonians E_R + E_L + lambda u whose lambdas are exchanged on the device (s.4o).  Every driver has `minimise()`:
FIRE for all its replicas, each with state and convergence of its own, in two more launches of libagbnp_md.so around the same
evaluation (back: judge and decide the move, front: move and tethers; s.4l), the host reading only every `check_every`
iterations.  Written in torch operations a step is seventeen launches around the six of the AGBNP evaluation
(`DeviceMD(fused=False)`, kept as the cross-check of the kernels): 0.163 -> 0.11 ms per step of 1dwc.

PyTorch is plumbing here (device arrays, the graph capture API), not the product.
"""
import ctypes as C
import os

import numpy as np

from . import _lib

KB = 0.0083144626  # kJ/mol/K

MAX_REPLICAS = _lib.MAX_GROUP  # AGBNP_HIP_MAX_GROUP

# the last word of a Philox counter names the stream (csrc/md_kernels.hip: kNoiseWord0, kNoiseWord1, kExchangeWord, kHamiltonianWord,
# kLambdaWord)
PHILOX_NOISE_0, PHILOX_NOISE_1, PHILOX_EXCHANGE, PHILOX_HAMILTONIAN, PHILOX_LAMBDA = 0, 1, 2, 3, 4

_M64 = 0xFFFFFFFFFFFFFFFF


class _GroupArgs(C.Structure):  # AgbnpMdGroup
    _fields_ = [("n", C.c_int), ("replicas", C.c_int), ("x", C.c_void_p), ("v", C.c_void_p), ("f", C.c_void_p), ("x0", C.c_void_p),
                ("hdt_m", C.c_void_p), ("mass", C.c_void_p), ("kT", C.c_void_p), ("seeds", C.c_void_p), ("c1", C.c_double),
                ("dt", C.c_double), ("ktether", C.c_double), ("energy", C.c_void_p), ("acc", C.c_void_p), ("done", C.c_void_p),
                ("log_pe", C.c_void_p), ("log_ke", C.c_void_p), ("step", C.c_void_p), ("capacity", C.c_longlong), ("last", C.c_void_p)]


class _ExchangeArgs(C.Structure):  # AgbnpMdExchange
    _fields_ = [("n", C.c_int), ("replicas", C.c_int), ("v", C.c_void_p), ("kT", C.c_void_p), ("rung_of_replica", C.c_void_p),
                ("replica_at_rung", C.c_void_p), ("last", C.c_void_p), ("step", C.c_void_p), ("attempts", C.c_void_p),
                ("scale", C.c_void_p), ("log", C.c_void_p), ("log_capacity", C.c_longlong), ("seed", C.c_ulonglong)]


class _HamiltonianArgs(C.Structure):  # AgbnpMdHamiltonian
    _fields_ = [("n", C.c_int), ("replicas", C.c_int), ("x", C.c_void_p), ("v", C.c_void_p), ("kT", C.c_void_p),
                ("walker_at_rung", C.c_void_p), ("rung_of_walker", C.c_void_p), ("last", C.c_void_p), ("tether_part", C.c_void_p),
                ("cross", C.c_void_p), ("step", C.c_void_p), ("attempts", C.c_void_p), ("partner", C.c_void_p), ("scale", C.c_void_p),
                ("log", C.c_void_p), ("log_capacity", C.c_longlong), ("seed", C.c_ulonglong)]


class _LambdaArgs(C.Structure):  # AgbnpMdLambda
    _fields_ = [("replicas", C.c_int), ("lambda", C.c_void_p), ("rung_of_replica", C.c_void_p), ("replica_at_rung", C.c_void_p),
                ("kT", C.c_void_p), ("u", C.c_void_p), ("step", C.c_void_p), ("attempts", C.c_void_p), ("log", C.c_void_p),
                ("log_capacity", C.c_longlong), ("seed", C.c_ulonglong)]


class _FireArgs(C.Structure):  # AgbnpMdFire
    _fields_ = [("w", C.c_void_p), ("dt", C.c_void_p), ("alpha", C.c_void_p), ("npos", C.c_void_p), ("iterations", C.c_void_p),
                ("converged", C.c_void_p), ("voids", C.c_void_p), ("fmax", C.c_void_p), ("coef", C.c_void_p), ("part", C.c_void_p),
                ("arrived", C.c_void_p), ("log_e", C.c_void_p), ("log_fmax", C.c_void_p), ("capacity", C.c_longlong),
                ("dt_max", C.c_double), ("f_inc", C.c_double), ("f_dec", C.c_double), ("alpha0", C.c_double), ("f_alpha", C.c_double),
                ("n_min", C.c_int), ("tolerance", C.c_double), ("max_move", C.c_double)]


GROUP_SYMBOLS = ("agbnp_md_group_pre", "agbnp_md_group_mid", "agbnp_md_group_post", "agbnp_md_group_tethers", "agbnp_md_exchange")
HAMILTONIAN_SYMBOLS = ("agbnp_md_hamiltonian_exchange",)
FIRE_SYMBOLS = ("agbnp_md_fire_back", "agbnp_md_fire_front")
LAMBDA_SYMBOLS = ("agbnp_md_lambda_exchange",)

# FIRE's constants (Bitzek et al., PRL 97, 170201) and the bounds of the move
FIRE_F_INC, FIRE_F_DEC, FIRE_ALPHA0, FIRE_F_ALPHA, FIRE_N_MIN = 1.1, 0.5, 0.1, 0.99, 5
JUMP_THRESHOLD = 0.04     # nm: a heavy atom that moves further between two evaluations gets that evaluation withheld
MAX_MOVE_LIMIT = 0.02     # nm: the largest `max_move` minimise() accepts, half the threshold

# one record per replica of what minimise() returns; energy (kJ/mol) and fmax (kJ/mol/nm) are those of the final positions
MINIMISE_RECORD = np.dtype([("iterations", "<i8"), ("converged", "<i4"), ("fmax", "<f8"), ("energy", "<f8"), ("voids", "<i4"),
                            ("withheld", "<i8")])

_vp, _gp = C.c_void_p, C.POINTER(_GroupArgs)
# every symbol of libagbnp_md.so the drivers call: name -> arguments (every result is an int: 0, or a hipError)
_SIGNATURES = {
    "agbnp_md_blocks": [C.c_int],
    "agbnp_md_group_pre": [_gp, C.c_int, _vp, _vp],
    "agbnp_md_group_mid": [_gp, C.c_int, _vp, _vp, _vp],
    "agbnp_md_group_post": [_gp, _vp, _vp],
    "agbnp_md_group_tethers": [_gp, _vp, _vp],
    "agbnp_md_exchange": [C.POINTER(_ExchangeArgs), _vp],
    "agbnp_md_hamiltonian_exchange": [C.POINTER(_HamiltonianArgs), _vp],
    "agbnp_md_lambda_exchange": [C.POINTER(_LambdaArgs), _vp],
    "agbnp_md_fire_back": [_gp, C.POINTER(_FireArgs), _vp, _vp],
    "agbnp_md_fire_front": [_gp, C.POINTER(_FireArgs), _vp, _vp],
}

_MD_LIB = None


def _md_lib():
    """libagbnp_md.so (example support, not part of the drop-in boundary); built by csrc/Makefile next to the engine."""
    global _MD_LIB
    if _MD_LIB is None:
        _lib.load()  # (one HIP runtime per process: the engine's loader settles which)
        path = os.environ.get("AGBNP_HIP_MD_LIBRARY") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libagbnp_md.so")  # override: diagnostic builds only
        if not os.path.exists(path):
            raise ImportError(f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
        lib = C.CDLL(path)
        for name, argtypes in _SIGNATURES.items():
            getattr(lib, name).argtypes = argtypes  # AttributeError if the library does not export it
        _MD_LIB = lib
    return _MD_LIB


def _check(rc):
    if rc != 0:
        raise RuntimeError(f"libagbnp_md.so: launch failed (hipError {rc})")


def _check_engine(rc, symbol, error_handle=None):
    """A return code of the engine (libagbnp_hip.so) in a driver's launch sequence: a failure raises with the library's message for
    `error_handle` behind the call's name."""
    if rc != _lib.OK:
        raise RuntimeError(f"{symbol}: " + _lib.last_error(error_handle))


_KINDS = {"langevin": 0, "verlet": 1}  # the kernels' `kind`


def _args(struct, **fields):
    """An argument struct filled by field name; a device tensor stands for its address.  A name that is not a field of
    `struct`, or a field left out, is an error here rather than a misplaced pointer in a kernel."""
    names = {name for name, _ in struct._fields_}
    if set(fields) != names:
        raise TypeError(f"{struct.__name__}: not a field {sorted(set(fields) - names)}, missing {sorted(names - set(fields))}")
    return struct(**{name: val.data_ptr() if hasattr(val, "data_ptr") else val for name, val in fields.items()})


def _on_side(torch, side, fn):
    """fn() enqueued on the stream `side` behind torch's current one, and waited for; returns what fn returns."""
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = fn()
    side.synchronize()
    return out


def _check_minimise(tolerance, max_iterations, check_every, dt0, dt_max, max_move):
    """minimise()'s arguments, judged before any device call."""
    if not 0.0 < float(max_move) <= MAX_MOVE_LIMIT:
        raise ValueError(f"minimise: max_move must be in (0, {MAX_MOVE_LIMIT}] nm, not {max_move}: the engine withholds an evaluation "
                         f"whose heavy atoms moved more than {JUMP_THRESHOLD} nm since the last one, and a move is kept to half of that")
    if not 0.0 < float(tolerance) < float("inf"):
        raise ValueError(f"minimise: tolerance must be positive and finite (kJ/mol/nm), not {tolerance}")
    if not 0.0 < float(dt0) < float("inf"):
        raise ValueError(f"minimise: dt0 must be positive and finite (ps), not {dt0}")
    if not float(dt0) <= float(dt_max) < float("inf"):
        raise ValueError(f"minimise: dt0 = {dt0} ps exceeds dt_max = {dt_max} ps")
    if int(max_iterations) < 1 or int(check_every) < 1:
        raise ValueError(f"minimise: max_iterations and check_every must be at least 1, not {max_iterations} and {check_every}")


class _Replicas:
    """The integrator state of R replicas of one system and the launches that advance it (csrc/md_kernels.hip).  State is
    strided -- x, v, frc [R][n][3], everything per replica [R]... -- so replica r's buffers are fixed slices and the kernels'
    argument struct is filled once.  Replica r starts at the system's positions with velocities drawn at temperatures[r] by a
    generator seeded seeds[r]; seeds[r] also keys its Philox stream.  The force evaluation between the launches is the
    driver's: `evaluate(stream)` adds forces to frc[r] and energies to e_agbnp[r]."""

    def __init__(self, torch, system, temperatures, seeds, k_tether, dt, friction, device, log_capacity):
        self.lib = lib = _md_lib()
        self.R, self.n = R, n = len(temperatures), int(system.n)
        self.dev = torch.device(device)
        self.dt, self.k, self.gamma = float(dt), float(k_tether), float(friction)
        self.c1 = float(np.exp(-self.gamma * self.dt))
        self.log_capacity = cap = int(log_capacity)
        f64 = dict(dtype=torch.float64, device=self.dev)
        i64 = dict(dtype=torch.int64, device=self.dev)
        # masses in amu: hydrogens 1.008, heavy atoms carbon-like (the .dat fixtures carry no element)
        self.mass1 = torch.tensor(np.where(system.ishydrogen == 1, 1.008, 12.0), **f64).contiguous()
        self.mass = self.mass1.reshape(-1, 1)
        self.hdt_m1 = ((0.5 * self.dt) / self.mass1).contiguous()  # dt / 2m
        self.x0 = torch.tensor(system.pos, **f64).contiguous()
        self.x = self.x0.unsqueeze(0).repeat(R, 1, 1).contiguous()
        self.v = torch.empty_like(self.x)
        for r in range(R):
            gen = torch.Generator(device=self.dev)
            gen.manual_seed(seeds[r])
            self.v[r] = torch.randn((n, 3), generator=gen, **f64) * torch.sqrt(KB * temperatures[r] / self.mass)
        self.frc = torch.zeros_like(self.x)
        self.kT = torch.tensor([KB * t for t in temperatures], **f64)  # bath temperatures, kJ/mol: an exchange swaps them
        self.seed_words = torch.tensor(np.array([s & _M64 for s in seeds], dtype=np.uint64).view(np.int64), **i64)
        self.e_agbnp = torch.zeros(R, **f64)  # the words the engine adds the AGBNP energies to (handed back as zeros by every step)
        blocks = int(lib.agbnp_md_blocks(n))
        # the tether energy as per-block partials (a run of steps alternates between the two: k_md_group_mid)
        self.parts = (torch.zeros((R, blocks), **f64), torch.zeros((R, blocks), **f64))
        self.acc = torch.zeros((R, 2), **f64)  # the kinetic-energy accumulators and the arrival counters of the back half
        self.done = torch.zeros(R, dtype=torch.int32, device=self.dev)
        # per-step logs written by the kernels: potential and kinetic energy at index `counter`
        self.log_pe = torch.zeros((R, cap), **f64)
        self.log_ke = torch.zeros((R, cap), **f64)
        self.counter = torch.zeros(R, **i64)
        self.last = torch.zeros((R, 2), **f64)  # {potential, kinetic} energy of every replica's last step
        self._g = _args(_GroupArgs, n=n, replicas=R, x=self.x, v=self.v, f=self.frc, x0=self.x0, hdt_m=self.hdt_m1, mass=self.mass1,
                        kT=self.kT, seeds=self.seed_words, c1=self.c1, dt=self.dt, ktether=self.k, energy=self.e_agbnp, acc=self.acc,
                        done=self.done, log_pe=self.log_pe, log_ke=self.log_ke, step=self.counter, capacity=cap, last=self.last)
        self._parts = (self.parts[0].data_ptr(), self.parts[1].data_ptr())
        self.part_read = 0  # the partial buffer last[:, 0] was summed from: 0 behind forces(), (s - 1) % 2 behind steps(.., s, ..)
        self.fire = None    # the minimiser's device words: allocated by the first minimise()

    def tethers(self, st):
        """f = -k (x - x0) of every replica, the tethers' energy as partials in parts[0]."""
        _check(self.lib.agbnp_md_group_tethers(C.byref(self._g), self._parts[0], st))

    def forces(self, torch, st, evaluate):
        """Tethers + AGBNP of every replica at the current positions, enqueued on `st` (torch's current stream): frc[r],
        last[r, 0]."""
        self.e_agbnp.zero_()
        self.tethers(st)
        evaluate(st)
        self._evaluated(torch)

    def _evaluated(self, torch):
        """The evaluation at the current positions is complete (tethers in parts[0], AGBNP in e_agbnp): last[:, 0] is their sum."""
        torch.add(self.parts[0].sum(dim=1), self.e_agbnp, out=self.last[:, 0])
        self.e_agbnp.zero_()  # (a step that follows starts its own sum)
        self.part_read = 0

    def steps(self, kind, steps, st, evaluate):
        """`steps` consecutive steps of all replicas: front halves, then (evaluation, back halves + next front halves in ONE
        launch) between the steps, evaluation, back halves: two launches around the only evaluation of a single step, one more
        than the evaluation's for every further one."""
        lib, g, parts = self.lib, C.byref(self._g), self._parts
        _check(lib.agbnp_md_group_pre(g, kind, parts[0], st))
        for j in range(steps):
            evaluate(st)
            if j + 1 < steps:
                _check(lib.agbnp_md_group_mid(g, kind, parts[j % 2], parts[(j + 1) % 2], st))
            else:
                _check(lib.agbnp_md_group_post(g, parts[j % 2], st))
        self.part_read = (steps - 1) % 2

    def _fire_state(self, torch, capacity):
        """The minimiser's device words, allocated at the first minimise() (the logs again when a later one asks for more)."""
        R, n = self.R, self.n
        fire = self.fire
        if fire is None:
            f64 = dict(dtype=torch.float64, device=self.dev)
            i32 = dict(dtype=torch.int32, device=self.dev)
            blocks = int(self.lib.agbnp_md_blocks(n))
            fire = dict(w=torch.zeros((R, n, 3), **f64), dt=torch.zeros(R, **f64), alpha=torch.zeros(R, **f64), npos=torch.zeros(R, **i32),
                        iterations=torch.zeros(R, dtype=torch.int64, device=self.dev), converged=torch.zeros(R, **i32),
                        voids=torch.zeros(R, **i32), fmax=torch.zeros(R, **f64), coef=torch.zeros((R, 4), **f64),
                        part=torch.zeros((R, blocks, 4), **f64), arrived=torch.zeros(R, **i32), capacity=0)
            self.fire = fire
        if capacity > fire["capacity"]:
            fire["log_e"] = torch.zeros((R, capacity), dtype=torch.float64, device=self.dev)
            fire["log_fmax"] = torch.zeros((R, capacity), dtype=torch.float64, device=self.dev)
            fire["capacity"] = capacity
        return fire

    def minimise(self, torch, st, evaluate, finish, tolerance=10.0, max_iterations=1000, check_every=50, dt0=0.001, dt_max=0.005,
                 max_move=0.01, on_check=None):
        """FIRE (csrc/md_kernels.hip) from the current positions, every replica with state and convergence of
        its own, enqueued on `st` (torch's current stream): tethers and an evaluation, then per iteration the back half (judge
        the evaluation, decide the move), the front half (move, tethers) and `evaluate(st)`.  Every `check_every` iterations
        `finish()` (withheld evaluations per member since its last call; it waits for the stream) and the `converged` words are
        read -- the only host reads before the end -- and `on_check(converged)` is called; it stops when every replica has
        converged or after `max_iterations`.  No atom moves more than `max_move` nm in an iteration.  v, counter, log_pe and
        log_ke are not touched; frc, last[:, 0], e_agbnp and part_read are left as forces() leaves them.  Returns one
        MINIMISE_RECORD per replica.  An evaluation the engine withheld (or one whose forces are not numbers) makes a void
        iteration for that replica, converged or not: counted in `voids`, repeated in place; `withheld` is what the members'
        finish() reported.  Where either is not zero the LAST evaluation may have been such a one: `energy`, `fmax`, frc and
        last[:, 0] of that replica then lack the AGBNP term, and forces() puts them right."""
        _check_minimise(tolerance, max_iterations, check_every, dt0, dt_max, max_move)  # (the drivers' too: theirs comes first)
        max_iterations, check_every = int(max_iterations), int(check_every)
        lib, g, part = self.lib, C.byref(self._g), self._parts[0]
        fire = self._fire_state(torch, max_iterations)
        for key in ("w", "npos", "iterations", "converged", "voids", "fmax", "coef", "arrived", "log_e", "log_fmax"):
            fire[key].zero_()
        fire["dt"].fill_(float(dt0))
        fire["alpha"].fill_(FIRE_ALPHA0)
        q = C.byref(_args(_FireArgs, **fire, dt_max=float(dt_max), f_inc=FIRE_F_INC, f_dec=FIRE_F_DEC, alpha0=FIRE_ALPHA0,
                          f_alpha=FIRE_F_ALPHA, n_min=FIRE_N_MIN, tolerance=float(tolerance), max_move=float(max_move)))
        self.e_agbnp.zero_()
        self.tethers(st)
        evaluate(st)
        withheld = np.zeros(self.R, dtype=np.int64)
        done = 0
        while done < max_iterations:
            chunk = min(check_every, max_iterations - done)
            for _ in range(chunk):
                _check(lib.agbnp_md_fire_back(g, q, part, st))
                _check(lib.agbnp_md_fire_front(g, q, part, st))
                evaluate(st)
            done += chunk
            withheld += np.asarray(finish(), dtype=np.int64).reshape(-1)
            converged = fire["converged"].cpu().numpy()
            if on_check:
                on_check(converged)
            if converged.all():
                break
        # as forces() ends: every replica's last evaluation is at the positions it now holds (a converged one's repeats the
        # evaluation it converged on)
        self._evaluated(torch)
        out = np.zeros(self.R, dtype=MINIMISE_RECORD)
        out["iterations"], out["converged"] = fire["iterations"].cpu().numpy(), fire["converged"].cpu().numpy()
        out["fmax"] = self.frc.square().sum(dim=2).max(dim=1).values.sqrt().cpu().numpy()
        out["energy"], out["voids"], out["withheld"] = self.last[:, 0].cpu().numpy(), fire["voids"].cpu().numpy(), withheld
        return out

    def minimisation_log(self):
        """(energy[R][iterations], fmax[R][iterations]) of the last minimise(): what every judged evaluation logged, as numpy
        arrays padded with zeros behind a replica's own count."""
        fire = self.fire
        if fire is None:
            raise RuntimeError("minimisation_log: minimise() has not been called")
        count = min(int(fire["iterations"].max().item()), fire["capacity"])
        return fire["log_e"][:, :count].cpu().numpy(), fire["log_fmax"][:, :count].cpu().numpy()


def _settle(forces, withheld):
    """First evaluations (allocations, capacity negotiation, forest packing), until `withheld()` reports none; bounded."""
    for _ in range(8):
        for _ in range(3):
            forces()
        if not withheld():
            return
    raise RuntimeError("AGBNP capacity negotiation did not converge")


class DeviceMD:
    """One trajectory: a replica group of one around `kernel.execute_device`, replayed as HIP graphs."""

    def __init__(self, system, kernel, k_tether=2.0e4, dt=0.001, temperature=300.0, friction=1.0, seed=0, device="cuda:0",
                 log_capacity=200000, fused=True):
        import torch
        self.torch = torch
        self.fused = bool(fused)
        self.seed = int(seed)
        self.system, self.kernel = system, kernel
        self.T = float(temperature)
        self.core = core = _Replicas(torch, system, [self.T], [self.seed], k_tether, dt, friction, device, log_capacity)
        self.dev, self.n, self.log_capacity = core.dev, core.n, core.log_capacity
        self.dt, self.k, self.gamma, self.c1 = core.dt, core.k, core.gamma, core.c1
        # views into the core's arrays
        self.x, self.v, self.frc, self.x0, self.mass = core.x[0], core.v[0], core.frc[0], core.x0, core.mass
        self.last = core.last[0]   # {potential, kinetic} energy of the last step
        self.ene = self.last[0:1]  # potential energy of the last force evaluation (tethers + AGBNP)
        self.log_pe, self.log_ke, self.counter = core.log_pe[0], core.log_ke[0], core.counter
        # The step in torch operations (`fused=False`, and the minimiser's record).  Every torch op below is one tiny launch (~2 us
        # each inside the replayed graph), so the step is written with as few of them as the arithmetic allows: fused
        # multiply-adds, preallocated outputs, dot products for the sums.
        f64 = dict(dtype=torch.float64, device=self.dev)
        self.hdt_m = core.hdt_m1.reshape(-1, 1)
        self.c2 = torch.sqrt((1.0 - self.c1 * self.c1) * KB * self.T / self.mass)
        self.noise = torch.empty_like(self.x)
        self.one = torch.ones(1, dtype=torch.int64, device=self.dev)
        self.d = torch.zeros_like(self.x)   # x - x0
        self.mv = torch.zeros_like(self.x)  # m v
        self.ke = torch.zeros(1, **f64)
        self._eager = None
        self.graphs = {}
        self.generation = None
        self.steps_done = 0

    # ---- force field: tethers + AGBNP (added on the device by the engine)
    def _evaluate(self, st):
        self.kernel.execute_device(self.x.data_ptr(), self.frc.data_ptr(), self.core.e_agbnp.data_ptr(), st)

    def forces(self):
        """Tethers + AGBNP at the current positions: self.frc, self.ene.  Inside a graph capture it joins the capture; called
        eagerly on torch's default (null) stream it runs on a stream of its own and waits for it -- the engine takes a null
        stream for its context's own stream, which nothing of torch's is ordered against."""
        torch = self.torch
        if not torch.cuda.is_current_stream_capturing() and torch.cuda.current_stream().cuda_stream == 0:
            return _on_side(torch, self._side(), self._forces)
        self._forces()

    def _side(self):
        if self._eager is None:
            self._eager = self.torch.cuda.Stream(device=self.dev)
        return self._eager

    def _forces(self):
        torch = self.torch
        st = torch.cuda.current_stream().cuda_stream
        if self.fused:
            return self.core.forces(torch, st, self._evaluate)
        torch.sub(self.x, self.x0, out=self.d)
        torch.mul(self.d, -self.k, out=self.frc)
        torch.mul(torch.dot(self.d.view(-1), self.d.view(-1)).reshape(1), 0.5 * self.k, out=self.ene)
        self.kernel.execute_device(self.x.data_ptr(), self.frc.data_ptr(), self.ene.data_ptr(), st)

    def _record(self):
        torch = self.torch
        torch.mul(self.v, self.mass, out=self.mv)
        torch.mul(torch.dot(self.mv.view(-1), self.v.view(-1)).reshape(1), 0.5, out=self.ke)
        self.log_pe.index_copy_(0, self.counter, self.ene)
        self.log_ke.index_copy_(0, self.counter, self.ke)
        self.counter.add_(self.one)

    def _fused_steps(self, kind, steps=1):
        """`steps` steps of the core on the current stream (csrc/md_kernels.hip): 8 launches for one, 7 for each further one."""
        self.core.steps(_KINDS[kind], steps, self.torch.cuda.current_stream().cuda_stream, self._evaluate)

    def step_verlet(self):  # velocity Verlet (the reference's NVE check uses OpenMM's VerletIntegrator, test_agbnp.py:57)
        if self.fused:
            return self._fused_steps("verlet")
        self.v.addcmul_(self.frc, self.hdt_m)
        self.x.add_(self.v, alpha=self.dt)
        self.forces()
        self.v.addcmul_(self.frc, self.hdt_m)
        self._record()

    def step_langevin(self):  # BAOAB (the reference uses LangevinIntegrator(300 K, 1/ps), test_agbnp.py:37, 1dwc_benchmark.py:20)
        if self.fused:
            return self._fused_steps("langevin")
        self.v.addcmul_(self.frc, self.hdt_m)
        self.x.add_(self.v, alpha=0.5 * self.dt)
        self.noise.normal_(generator=None)
        self.v.mul_(self.c1).addcmul_(self.c2, self.noise)
        self.x.add_(self.v, alpha=0.5 * self.dt)
        self.forces()
        self.v.addcmul_(self.frc, self.hdt_m)
        self._record()

    def step_descent(self, gain=2.0e-6):  # crude minimiser: a capped move along the force
        move = (gain * self.frc).clamp_(-0.002, 0.002)
        self.x.add_(move)
        self.forces()
        self._record()

    def minimise(self, tolerance=10.0, max_iterations=1000, check_every=50, dt0=0.001, dt_max=0.005, max_move=0.01, on_check=None):
        """FIRE from the current positions until the largest per-atom force norm (tethers + AGBNP) is below `tolerance`
        (kJ/mol/nm) or `max_iterations` have run (`_Replicas.minimise`): eager, on a stream of the driver's own, two launches of
        libagbnp_md.so around `execute_device` per iteration, the host reading only every `check_every` iterations.  No atom
        moves more than `max_move` nm between two evaluations, so none is withheld for a jump.  self.v and the step logs are
        untouched, and the state is as forces() leaves it: run() may follow.  Returns one MINIMISE_RECORD (a numpy array of 1)."""
        _check_minimise(tolerance, max_iterations, check_every, dt0, dt_max, max_move)
        torch, side = self.torch, self._side()
        return _on_side(torch, side, lambda: self.core.minimise(
            torch, side.cuda_stream, self._evaluate, lambda: [self.kernel.finish(side.cuda_stream)], tolerance, max_iterations,
            check_every, dt0, dt_max, max_move, on_check))

    # ---- graph capture / replay
    def settle(self):
        """Outside any capture: first evaluations (allocations, capacity negotiation, forest packing)."""
        torch = self.torch
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            _settle(self.forces, lambda: self.kernel.finish(side.cuda_stream))
        torch.cuda.synchronize()

    def _graph(self, kind, steps=1):
        """A HIP graph of `steps` consecutive MD steps of the given kind (captured once per kind, length and engine generation)."""
        torch = self.torch
        if self.generation != self.kernel.generation():  # first use, or the capacity variant was raised: kernels are stale
            self.graphs.clear()
            self.generation = self.kernel.generation()
        if (kind, steps) not in self.graphs:
            step = {"verlet": self.step_verlet, "langevin": self.step_langevin, "descent": self.step_descent}[kind]
            counter0 = self.counter.clone()
            state = (self.x.clone(), self.v.clone(), self.frc.clone(), self.last.clone())
            side = torch.cuda.Stream()
            with torch.cuda.stream(side):  # torch wants a few eager runs on a side stream before a capture
                step()
                self.kernel.finish(side.cuda_stream)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                if self.fused and kind in _KINDS:
                    self._fused_steps(kind, steps)
                else:
                    for _ in range(steps):
                        step()
            torch.cuda.synchronize()
            # the capture itself does not run the steps, the warm-up did: put the state back
            for dst, src in zip((self.x, self.v, self.frc, self.last), state):
                dst.copy_(src)
            self.counter.copy_(counter0)
            self.graphs[(kind, steps)] = g
        return self.graphs[(kind, steps)]

    def run(self, nsteps, kind="langevin", check_every=1000, on_report=None, steps_per_graph=10):
        """Replays the captured steps (`steps_per_graph` MD steps per graph launch: the host's share of a launch is paid once
        for all of them); every `check_every` steps synchronises and reads the engine's overflow log.  Returns the number of
        steps whose AGBNP contribution was withheld (tree capacity exceeded): 0 in a healthy run."""
        torch = self.torch
        missed = 0
        done = 0
        while done < nsteps:
            chunk = min(check_every, nsteps - done)
            many = chunk // steps_per_graph if steps_per_graph > 1 else 0
            if many:
                g = self._graph(kind, steps_per_graph)
                for _ in range(many):
                    g.replay()
            rest = chunk - many * steps_per_graph
            if rest:
                g = self._graph(kind)
                for _ in range(rest):
                    g.replay()
            done += chunk
            self.steps_done += chunk
            missed += self.kernel.finish(torch.cuda.current_stream().cuda_stream)
            if on_report:
                on_report(self)
        return missed

    # ---- observables
    def energies(self, last=None):
        """(potential, kinetic) per recorded step as numpy arrays."""
        n = int(self.counter.item())
        pe, ke = self.log_pe[:n].cpu().numpy(), self.log_ke[:n].cpu().numpy()
        if last:
            pe, ke = pe[-last:], ke[-last:]
        return pe, ke

    def temperature(self):
        ke = 0.5 * float((self.mass * self.v * self.v).sum())
        return 2.0 * ke / (3 * self.system.n * KB)


# ---- replica exchange on top of the replica groups --------------------------------------------------------

_M32 = 0xFFFFFFFF


def philox4x32(counter4, key2):
    """Philox4x32-10 (Salmon et al., SC'11; Random123) in plain Python integers: what `philox4x32` of csrc/md_kernels.hip
    computes.  counter4: four 32-bit words, key2: two.  Returns the four output words."""
    c0, c1, c2, c3 = (int(c) & _M32 for c in counter4)
    k0, k1 = (int(k) & _M32 for k in key2)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & _M32, (p0 >> 32) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + 0x9E3779B9) & _M32, (k1 + 0xBB67AE85) & _M32
    return c0, c1, c2, c3


def uniform53(a, b):
    """The kernels' uniform deviate in (0, 1] from two 32-bit words: 53 bits, never zero (its logarithm is taken)."""
    u = (((int(a) & _M32) << 21) ^ ((int(b) & _M32) >> 11)) & ((1 << 53) - 1)
    return (float(u) + 1.0) * (1.0 / 9007199254740992.0)


def _attempt_uniform(rung, attempt, word, exchange_seed):
    """`attempt_uniform` of csrc/md_kernels.hip: counter (k, a lo, a hi, word), key exchange_seed."""
    a, s = int(attempt), int(exchange_seed)
    w = philox4x32((int(rung), a & _M32, (a >> 32) & _M32, word), (s & _M32, (s >> 32) & _M32))
    return uniform53(w[0], w[1])


def exchange_uniform(rung, attempt, exchange_seed):
    """The deviate attempt `attempt` uses for the rung pair (rung, rung + 1): counter (k, a lo, a hi, 2), key exchange_seed."""
    return _attempt_uniform(rung, attempt, PHILOX_EXCHANGE, exchange_seed)


def exchange_places(attempts, R):
    """The log place of the first record of attempt `attempts`, which is the number of records the attempts before it left:
    (a + 1) / 2 even ones with R / 2 pairs each and a / 2 odd ones with (R - 1) / 2 (`record_place` of csrc/md_kernels.hip)."""
    a, R = int(attempts), int(R)
    return ((a + 1) // 2) * (R // 2) + (a // 2) * ((R - 1) // 2)


def exchange_delta(kT_lo, kT_hi, U_lo, U_hi):
    """Delta of a temperature exchange between two replicas (kT in kJ/mol, potential energies in kJ/mol): the exchange is
    accepted iff log(u) <= Delta, u uniform in (0, 1] -- min(1, exp(Delta)), the Metropolis rule for swapping the baths."""
    return (1.0 / kT_lo - 1.0 / kT_hi) * (U_lo - U_hi)


# one record of the exchange log (AgbnpMdExchangeRecord, csrc/md_kernels.hip); energies and kT in kJ/mol, before the decision
EXCHANGE_RECORD = np.dtype([("attempt", "<i8"), ("step", "<i8"), ("rung", "<i4"), ("replica_lo", "<i4"), ("replica_hi", "<i4"),
                            ("accepted", "<i4"), ("U_lo", "<f8"), ("U_hi", "<f8"), ("kT_lo", "<f8"), ("kT_hi", "<f8"), ("u", "<f8")])


class _GroupMD:
    """What the exchange drivers share: the core around `agbnp_hip_execute_group` on a stream of the driver's own, eager
    (group calls are not captured).  Slot r's buffers are fixed slices of the strided arrays, so the group call's handle and
    pointer arrays are built once.  A driver adds its exchange: `exchange()` enqueues one attempt on `self.stream`.  A member
    is whatever the driver's `_evaluate` evaluates -- a HipCalcAGBNPForceKernel, or a BindingEnergy for BindingReplicaMD --: it
    has numParticles, a library handle behind _need() / _h, and finish(stream)."""

    def __init__(self, system, kernels, temperatures, seeds, exchange_seed, k_tether, dt, friction, device, log_capacity):
        who = type(self).__name__
        kernels, temperatures = list(kernels), [float(t) for t in temperatures]
        R = len(kernels)
        seeds = list(range(R)) if seeds is None else [int(s) for s in seeds]
        if len(temperatures) != R or len(seeds) != R:
            raise ValueError(f"{who}: {R} kernels, {len(temperatures)} temperatures and {len(seeds)} seeds")
        if not 1 <= R <= MAX_REPLICAS:
            raise ValueError(f"{who}: a group has 1 to {MAX_REPLICAS} replicas, not {R}")
        if any(int(k.numParticles) != int(system.n) for k in kernels):
            raise ValueError(f"{who}: every kernel must hold the system's {int(system.n)} particles")
        if len({id(k) for k in kernels}) != R:
            raise ValueError(f"{who}: the same kernel was given twice (one context per replica)")
        if any(not 0.0 < t < float("inf") for t in temperatures):
            raise ValueError(f"{who}: temperatures must be positive and finite")
        import torch
        self.torch = torch
        self.core = core = _Replicas(torch, system, temperatures, seeds, k_tether, dt, friction, device, log_capacity)
        self.system, self.kernels, self.R, self.n, self.dev = system, kernels, R, core.n, core.dev
        self.ladder = np.array(temperatures)  # the temperature of rung k
        self.seeds, self.exchange_seed = seeds, int(exchange_seed)
        self.dt, self.k, self.gamma, self.c1, self.log_capacity = core.dt, core.k, core.gamma, core.c1, core.log_capacity
        self.x, self.v, self.frc, self.x0, self.mass, self.kT = core.x, core.v, core.frc, core.x0, core.mass, core.kT
        self.log_pe, self.log_ke, self.counter, self.last = core.log_pe, core.log_ke, core.counter, core.last
        self.attempts = torch.zeros(1, dtype=torch.int64, device=self.dev)
        self.scale = torch.ones(R, dtype=torch.float64, device=self.dev)
        self.exchange_capacity = core.log_capacity
        # the group call's arguments never change: member r's buffers are slices of the strided arrays
        for k in kernels:
            k._need()
        vpR = C.c_void_p * R
        self._handles = vpR(*[k._h for k in kernels])
        self._pos = vpR(*[self.x[r].data_ptr() for r in range(R)])
        self._frc = vpR(*[self.frc[r].data_ptr() for r in range(R)])
        self._ene = vpR(*[core.e_agbnp[r:r + 1].data_ptr() for r in range(R)])
        self.stream = torch.cuda.Stream(device=self.dev)  # everything of this driver is enqueued here
        self.steps_done = 0

    # ---- launches
    def _evaluate(self, st):
        """agbnp_hip_execute_group of all members on stream `st`: forces and energies are added to frc[r], e_agbnp[r]."""
        _check_engine(_lib.load().agbnp_hip_execute_group(self._handles, self.R, self._pos, self._frc, self._ene, C.c_void_p(st)),
                      "agbnp_hip_execute_group", self.kernels[0]._h)

    def _chunk(self, steps, attempt_follows):
        """run() is about to enqueue `steps` steps (as many evaluations); `attempt_follows`: an exchange attempt comes right
        behind them.  Nothing here: for a driver whose attempt uses something of the chunk's last evaluation."""

    def finish(self):
        """Every member's finish() on the driver's stream: withheld evaluations per member since the last call."""
        st = self.stream.cuda_stream
        return np.array([k.finish(st) for k in self.kernels], dtype=np.int64)

    def forces(self):
        """Tethers + AGBNP of every slot at the current positions: frc[r], last[r, 0].  Waits for the result."""
        _on_side(self.torch, self.stream, lambda: self.core.forces(self.torch, self.stream.cuda_stream, self._evaluate))

    def minimise(self, tolerance=10.0, max_iterations=1000, check_every=50, dt0=0.001, dt_max=0.005, max_move=0.01, on_check=None):
        """FIRE for every slot from the positions it holds, each under its own context's parameters and with convergence of
        its own (`_Replicas.minimise`): eager on the driver's stream, two launches of libagbnp_md.so around
        `agbnp_hip_execute_group` per iteration for all R, the host reading only every `check_every` iterations.  A slot that has
        converged is not moved again while the others go on.  v, counter and the step logs are untouched, and the state is as
        forces() leaves it: run() or exchange() may follow.  Returns one MINIMISE_RECORD per slot."""
        _check_minimise(tolerance, max_iterations, check_every, dt0, dt_max, max_move)
        return _on_side(self.torch, self.stream, lambda: self.core.minimise(
            self.torch, self.stream.cuda_stream, self._evaluate, self.finish, tolerance, max_iterations, check_every, dt0, dt_max,
            max_move, on_check))

    def settle(self):
        """Outside any timing: first evaluations (allocations, capacity negotiation, forest packing, the group's argument
        blocks), until every member's finish() reports nothing withheld."""
        _settle(self.forces, lambda: self.finish().any())
        self.torch.cuda.synchronize()

    def run(self, nsteps, kind="langevin", exchange_every=0, check_every=1000, on_report=None):
        """`nsteps` steps of every slot (5 + 1 launches per step for all of them), an exchange attempt after every
        `exchange_every` of them (0: none); every `check_every` steps (and at the end) synchronises and reads every member's
        overflow log.  Returns, per member, the number of evaluations that were withheld (all zeros in a healthy run): a step
        without the AGBNP term for that slot alone -- an exchange decided on such a step used a potential energy without it."""
        torch = self.torch
        code = _KINDS[kind]
        exchange_every, check_every = int(exchange_every), max(1, int(check_every))
        st = self.stream.cuda_stream
        missed = np.zeros(self.R, dtype=np.int64)
        done = since_exchange = since_check = 0
        self.stream.wait_stream(torch.cuda.current_stream())
        while done < nsteps:
            chunk = min(nsteps - done, check_every - since_check)
            if exchange_every > 0:
                chunk = min(chunk, exchange_every - since_exchange)
            self._chunk(chunk, exchange_every > 0 and since_exchange + chunk == exchange_every)
            self.core.steps(code, chunk, st, self._evaluate)
            done += chunk
            since_exchange += chunk
            since_check += chunk
            self.steps_done += chunk
            if exchange_every > 0 and since_exchange == exchange_every:
                self.exchange()
                since_exchange = 0
            if since_check == check_every or done == nsteps:
                missed += self.finish()
                since_check = 0
                if on_report:
                    on_report(self)
        self.stream.synchronize()
        return missed

    # ---- observables (each waits for the driver's stream)
    def energies(self, last=None):
        """(potential[R, steps], kinetic[R, steps]) of the recorded steps as numpy arrays."""
        self.stream.synchronize()
        n = min(int(self.counter.max().item()), self.log_capacity)
        pe, ke = self.log_pe[:, :n].cpu().numpy(), self.log_ke[:, :n].cpu().numpy()
        if last:
            pe, ke = pe[:, -last:], ke[:, -last:]
        return pe, ke

    def _records(self, dtype):
        """One record per attempted pair, in the order of the attempts."""
        self.stream.synchronize()
        count = min(exchange_places(self.attempts.item(), self.R), self.exchange_capacity)
        raw = self.records[:count * dtype.itemsize].cpu().numpy()
        return raw.view(dtype).copy()

    def acceptance(self):
        """accepted / attempted per rung pair (k, k + 1), k = 0 .. R - 2 (nan where nothing was attempted)."""
        log = self.exchange_log()
        tried = np.bincount(log["rung"], minlength=self.R - 1)[:max(self.R - 1, 0)].astype(float)
        took = np.bincount(log["rung"], weights=log["accepted"] == 1, minlength=self.R - 1)[:max(self.R - 1, 0)]
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(tried > 0, took / tried, np.nan)


class ReplicaMD(_GroupMD):
    """Temperature replica exchange of R replicas of one system: DeviceMD's integrator and force field (tethers + AGBNP) for
    all replicas at once -- one launch of libagbnp_md.so in front of and one behind `agbnp_hip_execute_group`, six launches a
    step for all R -- and exchange attempts between neighbouring rungs of the temperature ladder decided on the device.

    Replica r is a conformation: x[r], v[r] and kernels[r] stay together for the whole run.  An accepted exchange swaps the
    two replicas' bath temperatures and rungs (and rescales their velocities by sqrt(T_new / T_old)); no position moves, so
    no evaluation is withheld for it and no argument block of the group is rewritten.  Eager: group calls are not captured."""

    def __init__(self, system, kernels, temperatures, seeds=None, exchange_seed=0, k_tether=2.0e4, dt=0.001, friction=1.0,
                 device="cuda:0", log_capacity=200000):
        super().__init__(system, kernels, temperatures, seeds, exchange_seed, k_tether, dt, friction, device, log_capacity)
        torch, R = self.torch, self.R
        self.rung_of_replica = torch.arange(R, dtype=torch.int32, device=self.dev)  # replica r starts on rung r
        self.replica_at_rung = torch.arange(R, dtype=torch.int32, device=self.dev)
        self.records = torch.zeros(self.exchange_capacity * EXCHANGE_RECORD.itemsize, dtype=torch.uint8, device=self.dev)
        self._e = _args(_ExchangeArgs, n=self.n, replicas=R, v=self.v, kT=self.kT, rung_of_replica=self.rung_of_replica,
                        replica_at_rung=self.replica_at_rung, last=self.last, step=self.counter, attempts=self.attempts, scale=self.scale,
                        log=self.records, log_capacity=self.exchange_capacity, seed=self.exchange_seed & _M64)

    def exchange(self):
        """One exchange attempt between neighbouring rungs, enqueued on the driver's stream (two launches, nothing read)."""
        _check(self.core.lib.agbnp_md_exchange(C.byref(self._e), self.stream.cuda_stream))

    def temperatures(self):
        """The current bath temperature (K) of every replica."""
        self.stream.synchronize()
        return self.kT.cpu().numpy() / KB

    def rungs(self):
        """rung_of_replica: the rung of the ladder every replica sits on."""
        self.stream.synchronize()
        return self.rung_of_replica.cpu().numpy()

    def exchange_log(self):
        """One record (EXCHANGE_RECORD) per attempted pair, in the order of the attempts."""
        return self._records(EXCHANGE_RECORD)


# ---- Hamiltonian replica exchange: the slots keep their contexts, the conformations move -----------------------


def hamiltonian_uniform(rung, attempt, exchange_seed):
    """The deviate attempt `attempt` uses for the rung pair (rung, rung + 1): counter (k, a lo, a hi, 3), key exchange_seed --
    word 3 keeps the stream apart from `exchange_uniform`'s."""
    return _attempt_uniform(rung, attempt, PHILOX_HAMILTONIAN, exchange_seed)


def hamiltonian_delta(kT_lo, kT_hi, P_lo, P_hi, T_lo, T_hi, C_lo, C_hi):
    """Delta of an exchange of conformations between the rungs lo and hi: beta_lo [U_lo(x_lo) - U_lo(x_hi)] + beta_hi [U_hi(x_hi)
    - U_hi(x_lo)] with U_k = tethers + A_k, from what the device holds: P the rung's total potential at its own conformation, T
    the tethers' share of it, C the cross energy A_k(partner's conformation).  Accepted iff log(u) <= Delta.  For one
    Hamiltonian (C_lo = P_hi - T_hi, C_hi = P_lo - T_lo) it is `exchange_delta`."""
    return ((P_lo - T_lo) - C_lo) / kT_lo + ((P_hi - T_hi) - C_hi) / kT_hi + (1.0 / kT_lo - 1.0 / kT_hi) * (T_lo - T_hi)


# one record of the Hamiltonian exchange log (AgbnpMdHamiltonianRecord, csrc/md_kernels.hip); everything BEFORE the decision;
# accepted: 1, 0, or -1 for a void pair (a cross energy was withheld: nothing moved)
HAMILTONIAN_RECORD = np.dtype([("attempt", "<i8"), ("step", "<i8"), ("rung", "<i4"), ("walker_lo", "<i4"), ("walker_hi", "<i4"),
                               ("accepted", "<i4"), ("P_lo", "<f8"), ("P_hi", "<f8"), ("T_lo", "<f8"), ("T_hi", "<f8"), ("C_lo", "<f8"),
                               ("C_hi", "<f8"), ("kT_lo", "<f8"), ("kT_hi", "<f8"), ("u", "<f8")])


class HamiltonianReplicaMD(_GroupMD):
    """Hamiltonian replica exchange of R rungs of one system: ReplicaMD's integrator and launches (5 + 1 per step for all R)
    with the roles reversed.  Slot k is rung k for the whole run: kernels[k] (contexts of one system whose gamma, vdw_alpha and
    charge may differ), kT[k], seeds[k], the buffers x[k], v[k], frc[k] and the logs of slot k never move, so log_pe / log_ke are
    per rung.  What moves is the conformation: an accepted exchange swaps the contents of x[lo] and x[hi], and of v[lo] and
    v[hi], each rescaled to its new bath; walker_at_rung / rung_of_walker (device, int32) follow them, walker w starting on rung
    w.  An attempt costs a round of cross energies (agbnp_hip_energy_group with the pairs' position pointers permuted, hinted
    with expect_jump), two launches of libagbnp_md.so and a full evaluation of all R behind them; run() counts the withheld
    cross-round and refresh evaluations in their member's sum."""

    def __init__(self, system, kernels, temperatures, seeds=None, exchange_seed=0, k_tether=2.0e4, dt=0.001, friction=1.0,
                 device="cuda:0", log_capacity=200000):
        super().__init__(system, kernels, temperatures, seeds, exchange_seed, k_tether, dt, friction, device, log_capacity)
        torch, R, core, kernels = self.torch, self.R, self.core, self.kernels
        self.walker_at_rung = torch.arange(R, dtype=torch.int32, device=self.dev)
        self.rung_of_walker = torch.arange(R, dtype=torch.int32, device=self.dev)
        self.partner = torch.full((R,), -1, dtype=torch.int32, device=self.dev)
        self.cross = torch.zeros(R, dtype=torch.float64, device=self.dev)  # the kernel hands every word it read back as zero
        self.records = torch.zeros(self.exchange_capacity * HAMILTONIAN_RECORD.itemsize, dtype=torch.uint8, device=self.dev)
        # one argument struct per tether-partial buffer, each filled once: the decision reads the one the last back half read
        self._h = tuple(_args(_HamiltonianArgs, n=self.n, replicas=R, x=self.x, v=self.v, kT=self.kT, walker_at_rung=self.walker_at_rung,
                              rung_of_walker=self.rung_of_walker, last=self.last, tether_part=part, cross=self.cross, step=self.counter,
                              attempts=self.attempts, partner=self.partner, scale=self.scale, log=self.records,
                              log_capacity=self.exchange_capacity, seed=self.exchange_seed & _M64) for part in core.parts)
        p = lambda t: t.data_ptr()  # noqa: E731
        # the cross round of the two attempt parities: the members of the pairs (k, k + 1), k = parity, parity + 2, ..., each at
        # the position buffer of its partner's slot, its energy added to cross[k]
        self._cross_round = []
        for parity in (0, 1):
            members = [r for k in range(parity, R - 1, 2) for r in (k, k + 1)]
            partners = [r + 1 if (r - parity) % 2 == 0 else r - 1 for r in members]
            vpM = C.c_void_p * max(len(members), 1)
            self._cross_round.append((members, vpM(*[kernels[r]._h for r in members]), vpM(*[p(self.x[q]) for q in partners]),
                                      vpM(*[p(self.cross[r:r + 1]) for r in members])))
        self._attempt = 0  # attempts enqueued: the device's counter without reading it

    def exchange(self):
        """One exchange attempt between neighbouring rungs, enqueued on the driver's stream; nothing is read and nothing waited
        for.  Cross round (hints, one energy-only group call over the members of the attempt's pairs with the position pointers
        permuted), decision and exchange of the conformations (two launches), refresh (hints again -- the masks sit at the
        partner's conformation after a rejection and the host does not know the verdict -- then tethers and one full group
        evaluation of all R: frc[k] and last[k, 0] are rung k's at what it now holds).  An attempt without a pair only counts."""
        torch = self.torch
        st = self.stream.cuda_stream
        members, handles, pos, ene = self._cross_round[self._attempt & 1]
        self._attempt += 1
        self.stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(self.stream):
            if not members:
                self.attempts.add_(1)
                return
            for r in members:
                self.kernels[r].expect_jump()
            _check_engine(_lib.load().agbnp_hip_energy_group(handles, len(members), pos, ene, C.c_void_p(st)),
                          "agbnp_hip_energy_group", self.kernels[members[0]]._h)
            _check(self.core.lib.agbnp_md_hamiltonian_exchange(C.byref(self._h[self.core.part_read]), st))
            for r in members:
                self.kernels[r].expect_jump()
            self.core.forces(torch, st, self._evaluate)

    def walkers(self):
        """walker_at_rung: the walker (the conformation that started on that rung) every rung now holds."""
        self.stream.synchronize()
        return self.walker_at_rung.cpu().numpy()

    def exchange_log(self):
        """One record (HAMILTONIAN_RECORD) per attempted pair, in the order of the attempts; accepted = -1 marks a void pair,
        which acceptance() counts as attempted."""
        return self._records(HAMILTONIAN_RECORD)


# ---- lambda replica exchange over a binding ladder: the replicas keep everything but lambda ------------------


def lambda_uniform(rung, attempt, exchange_seed):
    """The deviate attempt `attempt` uses for the rung pair (rung, rung + 1): counter (k, a lo, a hi, 4), key exchange_seed --
    word 4 keeps the stream apart from the other two exchanges'."""
    return _attempt_uniform(rung, attempt, PHILOX_LAMBDA, exchange_seed)


def lambda_delta(lambda_lo, lambda_hi, kT_lo, kT_hi, u_lo, u_hi):
    """Delta of an exchange of lambda between two replicas under E_lambda = E_R + E_L + lambda u (kT, u in kJ/mol): minus the
    change of E_lambda / kT summed over both, (lambda_lo - lambda_hi) (u_lo / kT_lo - u_hi / kT_hi).  Accepted iff
    log(uniform) <= Delta.  Formed as the kernel forms it: each quotient a double, then the difference, then the product."""
    return (lambda_lo - lambda_hi) * (u_lo / kT_lo - u_hi / kT_hi)


# one record of the lambda exchange log (AgbnpMdLambdaRecord, csrc/md_kernels.hip); everything BEFORE the decision; accepted: 1,
# 0, or -1 for a void pair (a u word was 0.0 or not finite: a withheld evaluation; nothing swapped)
LAMBDA_RECORD = np.dtype([("attempt", "<i8"), ("step", "<i8"), ("rung", "<i4"), ("replica_lo", "<i4"), ("replica_hi", "<i4"),
                          ("accepted", "<i4"), ("u_lo", "<f8"), ("u_hi", "<f8"), ("lambda_lo", "<f8"), ("lambda_hi", "<f8"),
                          ("kT_lo", "<f8"), ("kT_hi", "<f8"), ("uniform", "<f8")])


def _check_ladder(who, lambdas, R):
    """A lambda ladder: R finite values, strictly increasing (rung k -> lambda_k)."""
    try:
        ladder = [float(x) for x in lambdas]
    except (TypeError, ValueError):
        raise ValueError(f"{who}: the lambda ladder must be a list of numbers")
    if len(ladder) != R:
        raise ValueError(f"{who}: {R} bindings and {len(ladder)} lambdas")
    if any(not np.isfinite(x) for x in ladder):
        raise ValueError(f"{who}: lambdas must be finite")
    if any(b <= a for a, b in zip(ladder, ladder[1:])):
        raise ValueError(f"{who}: the lambda ladder must be strictly increasing")
    return ladder


class BindingReplicaMD(_GroupMD):
    """Replica exchange in lambda over E_lambda = E_R + E_L + lambda u (BEDAM, single decoupling) of R replicas of one
    complex: ReplicaMD's integrator and launches around ONE `agbnp_hip_binding_execute_group` over R BindingEnergy objects, whose
    lambdas are a device tensor of the driver's.  Replica r is a conformation: x[r], v[r], bindings[r] and its bath kT[r] stay
    together; an accepted exchange swaps the two replicas' lambda words and rungs, as ReplicaMD swaps baths.  frc[r] holds
    tethers + F_lambda and e_agbnp[r] takes E_lambda, so the step kernels, minimise(), forces(), settle() and the logs work as in
    the other drivers.

    E_lambda is linear in lambda: an attempt needs no cross evaluation, only u of every replica at its own positions, and that
    comes from the evaluation the steps made anyway -- of the steps an attempt follows, the last evaluation alone passes the u
    pointers.  exchange() is then ONE small launch of libagbnp_md.so (decision, swap, all R u words back to zero) and a full
    evaluation of all R as the refresh: F_lambda and last[:, 0] of a replica whose lambda changed are stale, and the
    host does not know the verdict.  No hint is needed (nothing jumps), nothing is read.  A pair with a withheld evaluation
    (its u word still zero) is void: recorded with accepted = -1, nothing swapped.  A binding whose u is identically zero
    (version 0, a ligand without a heavy atom) makes every pair void.  exchange() called by hand outside run() finds no u words:
    every pair is void -- use run(exchange_every=...)."""

    def __init__(self, system, bindings, lambdas, temperatures=300.0, seeds=None, exchange_seed=0, k_tether=2.0e4, dt=0.001,
                 friction=1.0, device="cuda:0", log_capacity=200000):
        from .AGBNPplugin import BindingEnergy
        who = type(self).__name__
        bindings = list(bindings)
        R = len(bindings)
        if not 1 <= R <= MAX_REPLICAS:
            raise ValueError(f"{who}: a group has 1 to {MAX_REPLICAS} replicas, not {R}")
        if any(not isinstance(b, BindingEnergy) for b in bindings):
            raise ValueError(f"{who}: members must be BindingEnergy objects")
        ladder = _check_ladder(who, lambdas, R)
        try:
            temperatures = [float(t) for t in temperatures]
        except TypeError:
            temperatures = [float(temperatures)] * R
        super().__init__(system, bindings, temperatures, seeds, exchange_seed, k_tether, dt, friction, device, log_capacity)
        torch = self.torch
        self.bindings = self.kernels
        self.lambda_ladder = np.array(ladder)  # lambda of rung k
        self.lam = torch.tensor(ladder, dtype=torch.float64, device=self.dev)  # lambda of replica r: the group's d_lambdas
        self.u = torch.zeros(R, dtype=torch.float64, device=self.dev)  # where an attempt's evaluation adds u of replica r
        self.rung_of_replica = torch.arange(R, dtype=torch.int32, device=self.dev)  # replica r starts on rung r
        self.replica_at_rung = torch.arange(R, dtype=torch.int32, device=self.dev)
        self.records = torch.zeros(self.exchange_capacity * LAMBDA_RECORD.itemsize, dtype=torch.uint8, device=self.dev)
        self._l = _args(_LambdaArgs, replicas=R, rung_of_replica=self.rung_of_replica, replica_at_rung=self.replica_at_rung, kT=self.kT,
                        u=self.u, step=self.counter, attempts=self.attempts, log=self.records, log_capacity=self.exchange_capacity,
                        seed=self.exchange_seed & _M64, **{"lambda": self.lam})
        self._u = (C.c_void_p * R)(*[self.u[r:r + 1].data_ptr() for r in range(R)])
        self._u_in = 0  # evaluations until the one that passes the u pointers (0: none is waited for)

    # ---- launches
    def _chunk(self, steps, attempt_follows):
        self._u_in = int(steps) if attempt_follows else 0

    def _evaluate(self, st):
        """agbnp_hip_binding_execute_group of all bindings on stream `st`: F_lambda and E_lambda are added to frc[r], e_agbnp[r];
        u is added to u[r] by the last evaluation in front of an attempt alone."""
        with_u = self._u_in == 1
        self._u_in = max(self._u_in - 1, 0)
        _check_engine(_lib.load().agbnp_hip_binding_execute_group(self._handles, self.R, self._pos, C.c_void_p(self.lam.data_ptr()),
                                                                  self._frc, self._ene, self._u if with_u else None, C.c_void_p(st)),
                      "agbnp_hip_binding_execute_group")

    def exchange(self):
        """One exchange attempt between neighbouring rungs, enqueued on the driver's stream; nothing is read and nothing waited
        for: the decision (one launch, which also hands all R u words back as zeros), then tethers and one full group evaluation
        of all R without u pointers as the refresh."""
        torch = self.torch
        st = self.stream.cuda_stream
        self._u_in = 0
        self.stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(self.stream):
            _check(self.core.lib.agbnp_md_lambda_exchange(C.byref(self._l), st))
            self.core.forces(torch, st, self._evaluate)

    # ---- observables
    def lambdas(self):
        """The current lambda of every replica."""
        self.stream.synchronize()
        return self.lam.cpu().numpy()

    def rungs(self):
        """rung_of_replica: the rung of the lambda ladder every replica sits on."""
        self.stream.synchronize()
        return self.rung_of_replica.cpu().numpy()

    def exchange_log(self):
        """One record (LAMBDA_RECORD) per attempted pair, in the order of the attempts; accepted = -1 marks a void pair, which
        acceptance() counts as attempted."""
        return self._records(LAMBDA_RECORD)
