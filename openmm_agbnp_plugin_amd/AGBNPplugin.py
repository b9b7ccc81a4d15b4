"""Host-side mirror of the reference's Python module `AGBNPplugin` (python/AGBNPPlugin.i:46-84) and of the
plugin's kernel interface, on top of the gfx950 engine's C ABI.

`AGBNPForce` keeps the reference's method names, argument order and meaning, defaults and error
behaviour (openmmapi/include/AGBNPForce.h:39-155, openmmapi/src/AGBNPForce.cpp:15-78).
`HipCalcAGBNPForceKernel` plays the role of a platform's `CalcAGBNPForceKernel`
(openmmapi/include/AGBNPKernels.h:19-47): initialize / execute / copyParametersToContext.
`AGBNPContext` is the small stand-in for the OpenMM Context + ForceImpl pair that the parity tests
and benchmarks need (OpenMM itself is not part of this path): it owns positions and calls the kernel
the way AGBNPForceImpl does (openmmapi/src/AGBNPForceImpl.cpp:27-46).

Every call into the library is made the same way: the library is looked up when the call is made, after the
argument checks, and a failure surfaces as an OpenMMException with the library's own message (`_Handle._call`, `_check`).
"""
import ctypes as C

import numpy as np

from . import _lib


# the planes of an energy decomposition, in the order of include/agbnp_hip.h (agbnp_hip_decompose_*)
DECOMPOSITION_TERMS = ("cavity", "vdw", "gb_self", "gb_pair")


class OpenMMException(Exception):
    """Same role as OpenMM::OpenMMException in the reference: every API error surfaces as this type."""


def _md_unit_system():
    """OpenMM's md_unit_system (nm, ps, amu, kJ/mol, e, K) if a units module is importable in this process."""
    for name in ("openmm.unit", "simtk.unit"):
        try:
            module = __import__(name, fromlist=["md_unit_system"])
            return module.md_unit_system
        except Exception:
            continue
    return "md_unit_system"


def _strip_units(value):
    """The SWIG layer of the reference accepts OpenMM unit Quantities for every double argument and hands the C++
    class the bare number in the MD unit system (python/AGBNPPlugin.i:3-4: OpenMM's swig/typemaps.i calls
    value_in_unit_system(md_unit_system)).  Duck-typed here: anything with that method is converted, plain numbers pass."""
    if hasattr(value, "value_in_unit_system"):
        return float(value.value_in_unit_system(_md_unit_system()))
    return float(value)


class AGBNPForce:
    # enum NonbondedMethod (openmmapi/include/AGBNPForce.h:44-59)
    NoCutoff = 0
    CutoffNonPeriodic = 1
    CutoffPeriodic = 2

    def __init__(self):
        # defaults of AGBNPForce::AGBNPForce() (openmmapi/src/AGBNPForce.cpp:15)
        self._particles = []
        self._method = AGBNPForce.NoCutoff
        self._cutoff = 1.0
        self._version = 1
        self._solvent_radius = 1.0 * float(np.float32(0.1))  # SOLVENT_RADIUS (1.0*ANG)
        self._force_group = 0
        self._cache = None  # the arrays of _arrays()

    def getNumParticles(self):
        return len(self._particles)

    @staticmethod
    def _row(radius, gamma, vdw_alpha, charge, ishydrogen):
        return [_strip_units(radius), _strip_units(gamma), _strip_units(vdw_alpha), _strip_units(charge), bool(ishydrogen)]

    def addParticle(self, radius, gamma, vdw_alpha, charge, ishydrogen):
        """radius nm, gamma kJ/mol/nm^2, vdw_alpha kJ/mol nm^3... (as the reference), charge e. Returns the index."""
        self._particles.append(self._row(radius, gamma, vdw_alpha, charge, ishydrogen))
        self._cache = None
        return len(self._particles) - 1

    def _check_index(self, index):
        if index < 0 or index >= len(self._particles):
            raise OpenMMException("Assertion failure: Index out of range")  # ASSERT_VALID_INDEX

    def setParticleParameters(self, index, radius, gamma, vdw_alpha, charge, ishydrogen):
        self._check_index(index)
        row = self._particles[index] = self._row(radius, gamma, vdw_alpha, charge, ishydrogen)
        cache = self._cache
        if cache is not None:  # the arrays that cross the boundary follow in place (updateParametersInContext after a sweep of these)
            for k in range(4):
                cache[k][index] = row[k]
            cache[4][index] = 1 if row[4] else 0

    def getParticleParameters(self, index):
        """Returns the tuple (radius, gamma, vdw_alpha, charge, ishydrogen), as the SWIG wrapper does."""
        self._check_index(index)
        return tuple(self._particles[index])

    def getNonbondedMethod(self):
        return self._method

    def setNonbondedMethod(self, method):
        self._method = int(method)

    def getCutoffDistance(self):
        return self._cutoff

    def setCutoffDistance(self, distance):
        self._cutoff = _strip_units(distance)

    def getSolventRadius(self):
        return self._solvent_radius

    def setVersion(self, agbnp_version):
        if 0 <= agbnp_version <= 2:
            self._version = int(agbnp_version)
        else:
            raise OpenMMException("AGBNPForce::setVersion(): illegal version number")

    def getVersion(self):
        return self._version

    def getForceGroup(self):
        return self._force_group

    def setForceGroup(self, group):
        self._force_group = int(group)

    def updateParametersInContext(self, context):
        context._update_parameters(self)

    # helpers for the engine boundary
    def _arrays(self):
        """The five parameter arrays as they cross the C ABI (built once, then kept up to date by setParticleParameters)."""
        cache = self._cache
        if cache is None:
            p = self._particles
            f = lambda k: np.ascontiguousarray([x[k] for x in p], dtype=np.float64)
            cache = self._cache = (f(0), f(1), f(2), f(3), np.ascontiguousarray([1 if x[4] else 0 for x in p], dtype=np.int32))
        return cache

    @classmethod
    def from_arrays(cls, radius, gamma, vdw_alpha, charge, ishydrogen, version=1):
        force = cls()
        force.setVersion(version)
        for r, g, a, q, h in zip(radius, gamma, vdw_alpha, charge, ishydrogen):
            force.addParticle(r, g, a, q, bool(h))
        return force


# ---- what crosses the C ABI -------------------------------------------------------------------------------------------------
def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def _ptr(p):
    """A raw pointer -- a device pointer, a stream -- given as an int; None and 0 are NULL."""
    return C.c_void_p(p or 0)


def _parameters(force):
    """The count and the five parameter arrays of a force, as the create and update calls take them."""
    r, g, a, q, h = force._arrays()
    return len(r), _dp(r), _dp(g), _dp(a), _dp(q), _ip(h)


def _forces_array(forces, n, refusal):
    if not (isinstance(forces, np.ndarray) and forces.dtype == np.float64 and forces.flags.c_contiguous and forces.size == 3 * n):
        raise OpenMMException(refusal)


def _partition(sets, num_sets, n):
    """A partition of n atoms as set_atom_sets() takes it (a kernel's, a BindingEnergy's), checked as the library checks it:
    (sets as an int32 array, num_sets); num_sets None: max(sets) + 1."""
    try:
        given = np.asarray(sets)
        sets = np.ascontiguousarray(given, dtype=np.int32).reshape(-1)
        exact = given.ndim == 1 and np.array_equal(sets, given)  # (no fraction, no wrap-around into the int)
    except (TypeError, ValueError, OverflowError):
        raise OpenMMException("set_atom_sets(): sets must be a list of set indices, one per atom")
    if not exact or sets.size != n:
        raise OpenMMException("set_atom_sets(): sets must hold one integer set index per atom")
    if num_sets is None:
        num_sets = int(sets.max()) + 1 if sets.size else 0
    num_sets = int(num_sets)
    if not 1 <= num_sets <= _lib.MAX_SETS:
        raise OpenMMException(f"set_atom_sets(): num_sets must be 1 .. {_lib.MAX_SETS}")
    if sets.min() < 0 or sets.max() >= num_sets:
        raise OpenMMException("set_atom_sets(): every set index must be 0 .. num_sets - 1")
    return sets, num_sets


def _parameter_sets(gamma, vdw_alpha, charge, n):
    """The parameter sets of set_parameter_sets() as they cross the C ABI, checked as the library checks them: three float64
    arrays [M, n] (a [n] array is one set), M 1 .. MAX_PARAMETER_SETS.  Returns (M, gamma, vdw_alpha, charge)."""
    tables = []
    for name, given in (("gamma", gamma), ("vdw_alpha", vdw_alpha), ("charge", charge)):
        try:
            a = np.ascontiguousarray(given, dtype=np.float64)
        except (TypeError, ValueError):
            raise OpenMMException(f"set_parameter_sets(): {name} must be an array of numbers, [M, N] or [N]")
        if a.ndim == 1:
            a = a.reshape(1, -1)
        if a.ndim != 2 or a.shape[1] != n:
            raise OpenMMException(f"set_parameter_sets(): {name} must be [M, N] or [N] with N = {n} particles")
        if not np.isfinite(a).all():
            raise OpenMMException(f"set_parameter_sets(): {name} must be finite")
        tables.append(a)
    m = tables[0].shape[0]
    if any(a.shape[0] != m for a in tables):
        raise OpenMMException("set_parameter_sets(): gamma, vdw_alpha and charge must hold the same number of sets")
    if not 1 <= m <= _lib.MAX_PARAMETER_SETS:
        raise OpenMMException(f"set_parameter_sets(): the number of sets must be 1 .. {_lib.MAX_PARAMETER_SETS}")
    return (m, *tables)


def _check(rc, error_handle=None):
    """A return code of the library: a failure raises with the message the library keeps for `error_handle` (None: the message
    of the calls that are not made on a context)."""
    if rc != _lib.OK:
        raise OpenMMException(_lib.last_error(error_handle))


class _Handle:
    """What HipCalcAGBNPForceKernel and BindingEnergy share: a library handle `_h` (None: there is none), the calls on it, the
    log of withheld evaluations, the partition of the matrix calls, the positions check and the release.  The symbols that
    differ are class data."""
    _NEED = _WITHHELD = _DESTROY = _SET_SETS = _NUM_SETS = None
    _OWN_ERRORS = True  # the library keeps the messages of this handle's calls under the handle (else: under None)
    _h = None
    _num_sets = 0  # S of the partition set through THIS object (pair_matrix_group() checks it before the library is reached)

    def _need(self):
        if self._h is None:
            raise OpenMMException(self._NEED)

    def _library(self):
        """For the calls whose result is not a return code."""
        self._need()
        return _lib.load()

    def _call(self, symbol, *args):
        """The one way of a method into the library: the handle is needed, `symbol` of _lib.load() is looked up now, after the
        caller's argument checks, and called on the handle; a failure raises with the library's message for this class."""
        if self._h is None:  # (_need() without its frame: every evaluation comes through here)
            raise OpenMMException(self._NEED)
        _check(getattr(_lib.load(), symbol)(self._h, *args), self._h if self._OWN_ERRORS else None)

    def _positions(self, positions, who):
        self._need()
        pos = np.ascontiguousarray(positions, dtype=np.float64).reshape(-1)
        if pos.size != 3 * self.numParticles:
            raise OpenMMException(f"{who}(): wrong number of positions")
        return pos

    def withheld(self):
        """Indices (enqueue order since the finish() before the last one) of the evaluations -- of a BindingEnergy: the binding
        evaluations -- the last finish() reported as withheld."""
        count = getattr(self._library(), self._WITHHELD)
        n = count(self._h, None, 0)
        idx = np.full(max(n, 1), -1, dtype=np.int32)  # the library fills as many indices as its log holds (it only COUNTS beyond bit 2047)
        count(self._h, _ip(idx), n)
        return [int(k) for k in idx if k >= 0]

    def set_atom_sets(self, sets, num_sets=None):
        """The partition of the atoms that pair_matrix() tabulates (include/agbnp_hip.h, agbnp_hip_set_atom_sets and
        agbnp_hip_binding_set_atom_sets): sets[i] in 0 .. num_sets - 1 is the set of atom i; sets need not be contiguous and may
        be empty; what a set is of is in the class's own text.  num_sets defaults to max(sets) + 1.  Replaces an earlier
        partition and survives copyParametersToContext(); changes nothing an evaluation reads.  The input is checked here,
        before the library is touched."""
        self._need()
        sets, num_sets = _partition(sets, num_sets, self.numParticles)
        self._call(self._SET_SETS, int(sets.size), _ip(sets), num_sets)
        self._num_sets = num_sets

    def num_atom_sets(self):
        """The number of sets of the partition in force; 0: none has been set."""
        return int(getattr(self._library(), self._NUM_SETS)(self._h))

    def release(self):
        if self._h is not None:
            getattr(_lib.load(), self._DESTROY)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


class HipCalcAGBNPForceKernel(_Handle):
    """The 'HIP platform' implementation of CalcAGBNPForceKernel.

    set_atom_sets(): a set is whatever pair_matrix() is to tabulate by -- an atom's residue, its chain, receptor or ligand."""
    _NEED = "HipCalcAGBNPForceKernel: initialize() has not been called"
    _WITHHELD, _DESTROY = "agbnp_hip_withheld_evaluations", "agbnp_hip_destroy"
    _SET_SETS, _NUM_SETS = "agbnp_hip_set_atom_sets", "agbnp_hip_num_atom_sets"
    _GROUP = ("group", "members", _lib.MAX_GROUP, False)  # what a group of these is called, its bound, members distinct

    @staticmethod
    def Name():
        return "CalcAGBNPForce"

    MODES = {"reference": 0, "fast": 1, "deterministic": 2, "fast+deterministic": 3, "fast+single": 5}

    def __init__(self, device=0, mode="reference"):
        """mode "reference" (default): the Reference platform's semantics, the parity target.  mode "fast": the
        OpenCL platform's semantics -- every pair stage truncated at the force's cutoff distance (include/agbnp_hip.h)."""
        self._h = None
        self._device = device
        self._mode = self.MODES[mode]
        self.numParticles = 0

    def initialize(self, force):
        self.release()
        parameters = _parameters(force)
        self.numParticles = parameters[0]
        handle = C.c_void_p()
        _check(_lib.load().agbnp_hip_create(C.byref(handle), *parameters, force.getVersion(), force.getNonbondedMethod(),
                                            force.getCutoffDistance(), self._device))
        self._h = handle
        self._num_sets = self._num_parameter_sets = 0  # (a new context has no partition and no parameter sets)
        if self._mode:
            self._call("agbnp_hip_set_mode", self._mode)

    def set_mode(self, mode):
        self._need()
        self._mode = self.MODES[mode]
        self._call("agbnp_hip_set_mode", self._mode)

    def execute(self, positions, forces, includeForces=True, includeEnergy=True):
        """CPU-platform convention of the reference: forces (N x 3 float64 array) are accumulated in place,
        the energy is returned.  includeForces/includeEnergy are accepted and ignored, as in the reference
        (ReferenceAGBNPKernels.cpp:139-149 always computes both)."""
        pos = self._positions(positions, "execute")
        _forces_array(forces, self.numParticles, "execute(): forces must be a C-contiguous float64 array of 3N values")
        e = C.c_double(0.0)
        self._call("agbnp_hip_execute_host", _dp(pos), _dp(forces), C.byref(e))
        return e.value

    def execute_device(self, d_positions, d_forces, d_energy, stream=None):
        """GPU-platform convention (reference OpenCL platform): raw FP64 device pointers (ints), forces and
        energy are ADDED on the device, nothing is returned.  Asynchronous; call finish().

        What a caller has to know (include/agbnp_hip.h, "Five-launch mode"): the tree launch finds every heavy atom's neighbours
        through masks laid down at an earlier evaluation, with a skin.  Positions that differ from the PREVIOUS evaluation's by
        more than 0.04 nm for some heavy atom (a minimiser's long step, a Monte-Carlo move, unrelated geometries one after the
        other) cost one withheld evaluation: finish() reports it, withheld() names it, running it again is right (execute(), the
        host-buffer entry point, repeats by itself).  MD steps are two orders of magnitude below that;
        AGBNP_HIP_FIVE_LAUNCHES=0 lifts the restriction for the price of one more launch per evaluation."""
        self._call("agbnp_hip_execute_device", C.c_void_p(d_positions), C.c_void_p(d_forces), C.c_void_p(d_energy), _ptr(stream))

    def execute_openmm(self, d_posq, posq_is_double, d_posq_correction, d_atom_index, padded_num_atoms, d_force_buffer,
                       d_energy_buffer, energy_is_double, energy_slot=0, stream=None):
        """The data conventions of an OpenMM GPU context (reference OpenCL platform): posq real4 in the context's
        atom order (+ optional float4 correction), atomIndex map, 2^32 fixed-point force planes, energy buffer slot.
        Raw device pointers (ints; 0 = NULL).  Asynchronous; call finish()."""
        self._call("agbnp_hip_execute_openmm", C.c_void_p(d_posq), int(bool(posq_is_double)), _ptr(d_posq_correction), _ptr(d_atom_index),
                   int(padded_num_atoms), C.c_void_p(d_force_buffer), _ptr(d_energy_buffer), int(bool(energy_is_double)),
                   int(energy_slot), _ptr(stream))

    def energy(self, positions):
        """Energy-only evaluation (what OpenMM asks for with includeForces=false): the energy execute() would return at
        these positions, computed without the force passes where the context allows it (include/agbnp_hip.h).  No forces
        are written anywhere; withheld evaluations are repeated inside, like execute()."""
        pos = self._positions(positions, "energy")
        e = C.c_double(0.0)
        self._call("agbnp_hip_energy_host", _dp(pos), C.byref(e))
        return e.value

    def energy_device(self, d_positions, d_energy, stream=None):
        """Energy-only form of execute_device(): the energy is ADDED to *d_energy on the device, nothing else is written.
        Asynchronous, counted in the same log as full evaluations (finish(), withheld(), poll(), wait_verdict()).  Refused
        (OpenMMException) inside a stream capture."""
        self._call("agbnp_hip_energy_device", C.c_void_p(d_positions), C.c_void_p(d_energy), _ptr(stream))

    def energy_openmm(self, d_posq, posq_is_double, d_posq_correction, d_atom_index, padded_num_atoms, d_energy_buffer,
                      energy_is_double, energy_slot=0, stream=None):
        """Energy-only form of execute_openmm(): no force buffer; the energy is ADDED to d_energy_buffer[energy_slot]."""
        self._call("agbnp_hip_energy_openmm", C.c_void_p(d_posq), int(bool(posq_is_double)), _ptr(d_posq_correction), _ptr(d_atom_index),
                   int(padded_num_atoms), C.c_void_p(d_energy_buffer), int(bool(energy_is_double)), int(energy_slot), _ptr(stream))

    def decompose(self, positions):
        """Per-atom decomposition of the energy at these positions (include/agbnp_hip.h, agbnp_hip_decompose_host): returns
        (energy, terms) with terms a float64 array [4, N] in the order of DECOMPOSITION_TERMS -- cavity, vdW, GB self, GB pair
        (each pair shared half and half) -- whose sum over everything is the energy.  Version 0 has the cavity plane only.  No
        forces are written anywhere; withheld evaluations are repeated inside, like energy()."""
        pos = self._positions(positions, "decompose")
        terms = np.zeros((len(DECOMPOSITION_TERMS), self.numParticles))
        e = C.c_double(0.0)
        self._call("agbnp_hip_decompose_host", _dp(pos), _dp(terms), C.byref(e))
        return e.value, terms

    def decompose_device(self, d_positions, d_per_atom, d_energy=None, stream=None):
        """Device-resident form of decompose(): the 4 N terms are ADDED to d_per_atom (term-major planes of N doubles, atom
        order) and the total to *d_energy when it is given; raw FP64 device pointers (ints).  Asynchronous, counted in the same
        log as every other evaluation (finish(), withheld(), poll(), wait_verdict()); a withheld one adds nothing.  Refused
        (OpenMMException) inside a stream capture."""
        self._call("agbnp_hip_decompose_device", C.c_void_p(d_positions), C.c_void_p(d_per_atom), _ptr(d_energy), _ptr(stream))

    def pair_matrix(self, positions):
        """Set-pair interaction matrix of the energy at these positions (include/agbnp_hip.h, agbnp_hip_pair_matrix_host):
        returns (energy, M) with M a float64 array [S, S] over the sets of set_atom_sets().  M[a, b] = M[b, a] is half the GB pair
        energy between sets a and b, M[a, a] what the set holds in itself (cavity, vdW, GB self, its own pairs); row a sums to
        the set's share of decompose()'s terms and M.sum() is the energy.  Withheld evaluations are repeated inside."""
        pos = self._positions(positions, "pair_matrix")
        s = self.num_atom_sets()
        matrix = np.zeros((max(s, 1), max(s, 1)))  # (no partition: the library refuses, with its message)
        e = C.c_double(0.0)
        self._call("agbnp_hip_pair_matrix_host", _dp(pos), _dp(matrix), C.byref(e))
        return e.value, matrix

    def pair_matrix_device(self, d_positions, d_matrix, d_energy=None, stream=None):
        """Device-resident form of pair_matrix(): the S S entries are ADDED to d_matrix (row-major FP64) and the total to
        *d_energy when it is given; raw device pointers (ints).  Asynchronous, counted in the same log as every other
        evaluation (finish(), withheld(), poll(), wait_verdict()); a withheld one adds nothing.  Refused (OpenMMException)
        inside a stream capture."""
        self._call("agbnp_hip_pair_matrix_device", C.c_void_p(d_positions), C.c_void_p(d_matrix), _ptr(d_energy), _ptr(stream))

    _num_parameter_sets = 0  # M of the sets set through THIS object (perturbed_energies_group() checks it before the library is reached)

    def set_parameter_sets(self, gamma, vdw_alpha, charge):
        """The parameter sets that perturbed_energies() scores (include/agbnp_hip.h, agbnp_hip_set_parameter_sets): float64
        arrays [M, N] -- or [N] for one set -- of gamma, vdw_alpha and charge, M 1 .. 16.  Radii and hydrogen flags are the
        kernel's own; a hydrogen's gamma counts as 0.  Replaces earlier sets and survives copyParametersToContext(); changes
        nothing an evaluation reads.  The shapes are checked here, before the library is touched."""
        self._need()
        m, g, a, q = _parameter_sets(gamma, vdw_alpha, charge, self.numParticles)
        self._call("agbnp_hip_set_parameter_sets", self.numParticles, m, _dp(g), _dp(a), _dp(q))
        self._num_parameter_sets = m

    def num_parameter_sets(self):
        """The number of parameter sets in force; 0: none have been set."""
        return int(self._library().agbnp_hip_num_parameter_sets(self._h))

    def perturbed_energies(self, positions):
        """The energy of these positions under every parameter set of set_parameter_sets(), from ONE evaluation
        (include/agbnp_hip.h, agbnp_hip_perturbed_energies_host): returns (energy, energies) with energy the kernel's own --
        what energy() returns -- and energies a float64 array [M], energies[m] what a kernel initialised with set m would
        return at these positions in this kernel's mode.  Withheld evaluations are repeated inside."""
        pos = self._positions(positions, "perturbed_energies")
        energies = np.zeros(max(self.num_parameter_sets(), 1))  # (no sets: the library refuses, with its message)
        e = C.c_double(0.0)
        self._call("agbnp_hip_perturbed_energies_host", _dp(pos), _dp(energies), C.byref(e))
        return e.value, energies

    def perturbed_energies_device(self, d_positions, d_energies, d_energy=None, stream=None):
        """Device-resident form of perturbed_energies(): the M energies are ADDED to d_energies and the kernel's own to *d_energy
        when it is given; raw FP64 device pointers (ints).  Asynchronous, counted in the same log as every other evaluation
        (finish(), withheld(), poll(), wait_verdict()); a withheld one adds nothing.  Refused (OpenMMException) inside a stream
        capture and without sets."""
        self._call("agbnp_hip_perturbed_energies_device", C.c_void_p(d_positions), C.c_void_p(d_energies), _ptr(d_energy), _ptr(stream))

    def atom_order_changed(self):
        """The context has reordered its atoms (same atomIndex array, new contents): the next execute_openmm() rebuilds the
        engine's maps first instead of losing one evaluation to the check on the device."""
        self._library().agbnp_hip_atom_order_changed(self._h)

    def expect_jump(self):
        """A hint: the positions of the NEXT evaluation are unrelated to the last ones (another replica's conformation, a
        restart).  That evaluation, through any entry point, lays the neighbour masks down at its own positions first -- one
        small launch, no synchronisation -- and is not withheld for the jump.  Consumed by that evaluation; does nothing where
        the context does not run the five-launch mode (include/agbnp_hip.h, agbnp_hip_expect_jump)."""
        self._call("agbnp_hip_expect_jump")

    def finish(self, stream=None):
        """Synchronise and read the device's overflow log: returns the number of evaluations enqueued since the
        previous finish() whose forces and energy were WITHHELD on the device (0 = all complete).  Those must be
        run again (see withheld()); the context has already switched to the packing / capacity variant they need."""
        rep = C.c_int(0)
        self._call("agbnp_hip_finish", _ptr(stream), C.byref(rep))
        return int(rep.value)

    def poll(self):
        """Non-blocking: (evaluations completed since the last finish(), how many of them were withheld), read from pinned
        host memory the device writes at the end of every evaluation (no device call)."""
        done, bad = C.c_int(0), C.c_int(0)
        if self._library().agbnp_hip_poll(self._h, C.byref(done), C.byref(bad)) != _lib.OK:
            raise OpenMMException("agbnp_hip_poll: no pinned status memory")
        return int(done.value), int(bad.value)

    def wait_verdict(self, evaluations=0, timeout=10.0):
        """The strict per-evaluation check without draining the stream: blocks this thread (no device call) until the device
        has delivered its verdict on every evaluation enqueued since the last finish() (or on `evaluations` of them) and
        returns (evaluations judged, how many were withheld).  The verdict of an evaluation is final when its tree stage
        has ended; its forces follow on the stream, gated on the device by the same words.  Raises on a timeout."""
        done, bad = C.c_int(0), C.c_int(0)
        verdict = self._library().agbnp_hip_wait_verdict(self._h, int(evaluations), float(timeout), C.byref(done), C.byref(bad))
        if verdict == _lib.ERR_TIMEOUT:
            raise OpenMMException(f"agbnp_hip_wait_verdict: timed out after {timeout} s with {int(done.value)} evaluation(s) judged")
        if verdict != _lib.OK:
            raise OpenMMException("agbnp_hip_wait_verdict: no pinned status memory")
        return int(done.value), int(bad.value)

    def generation(self):
        """Changes when a captured HIP graph of this context has gone stale (capacity variant raised; an evaluation through the
        other device-resident entry point than the graph's: include/agbnp_hip.h)."""
        return int(self._library().agbnp_hip_generation(self._h))

    def copyParametersToContext(self, force):
        self._need()
        self._call("agbnp_hip_update_parameters", *_parameters(force))

    # ---- diagnostics (test support) -------------------------------------------------------------
    SCALARS = dict(e_vol1=0, e_vol2=1, e_atom=2, e_gb_pair=3, max_subtree_nodes=4, total_nodes=5, variant=6, max_local_atoms=7, forests=8, rows_on=9, row_builds=10, pack_level=11, pack_age=12, row_slice=13, pack_plans=14, overflow_kinds=15, launches=16, healed_forests=17, energy_only_launches=18, group_members=19, last_evaluation_kind=20, group_block_writes=21)
    VECTORS = dict(selfvol_vdw=0, born=1, scale=2, selfvol_large=3, subtree_nodes=4, subtree_atoms=5)

    def scalar(self, name):
        self._need()
        v = C.c_double(0)
        self._call("agbnp_hip_get_scalar", self.SCALARS[name], C.byref(v))
        return v.value

    def vector(self, name):
        self._need()
        out = np.zeros(self.numParticles)
        self._call("agbnp_hip_get_vector", self.VECTORS[name], _dp(out))
        return out

    def tables(self):
        lib = self._library()
        ni, nj = C.c_int(0), C.c_int(0)
        lib.agbnp_hip_get_table_sizes(self._h, C.byref(ni), C.byref(nj))
        y = np.zeros(ni.value * nj.value * 16)
        y2 = np.zeros_like(y)
        ti = np.zeros(self.numParticles, dtype=np.int32)
        tj = np.zeros(self.numParticles, dtype=np.int32)
        lib.agbnp_hip_get_tables(self._h, _dp(y), _dp(y2), _ip(ti), _ip(tj))
        return dict(y=y.reshape(ni.value, nj.value, 16), y2=y2.reshape(ni.value, nj.value, 16), type_screened=ti, type_screener=tj)

    def set_diagnostics(self, enabled):
        """Collect the pass-1 (enlarged radii) self volumes too (vector 'selfvol_large')."""
        self._library().agbnp_hip_set_diagnostics(self._h, 1 if enabled else 0)

    def set_profiling(self, enabled):
        self._library().agbnp_hip_set_profiling(self._h, 1 if enabled else 0)

    def kernel_times(self):
        """{kernel name: (total ms, launches)} accumulated since set_profiling(True)."""
        lib = self._library()
        k = lib.agbnp_hip_num_kernels()
        ms = np.zeros(k)
        cnt = np.zeros(k, dtype=np.int64)
        lib.agbnp_hip_get_kernel_times(self._h, _dp(ms), cnt.ctypes.data_as(C.POINTER(C.c_long)))
        return {lib.agbnp_hip_kernel_name(i).decode(): (float(ms[i]), int(cnt[i])) for i in range(k)}


def _ligand_indices(ligand_atoms, n):
    """The ligand's atoms in ascending order, checked as agbnp_hip_binding_create checks them."""
    try:
        given = [int(a) for a in ligand_atoms]
    except (TypeError, ValueError):
        raise OpenMMException("BindingEnergy(): ligand_atoms must be a list of atom indices")
    if not 1 <= len(given) < n:
        raise OpenMMException(f"BindingEnergy(): the ligand has 1 to N - 1 = {n - 1} atoms, not {len(given)}")
    if min(given) < 0 or max(given) >= n:
        raise OpenMMException("BindingEnergy(): ligand atom index out of range")
    if len(set(given)) != len(given):
        raise OpenMMException("BindingEnergy(): a ligand atom index is given twice")
    return np.ascontiguousarray(sorted(given), dtype=np.int32)


class BindingEnergy(_Handle):
    """Binding-energy evaluations (include/agbnp_hip.h, agbnp_hip_binding_*): the complex, its receptor and its ligand in one
    call.  `force` holds the particles of the complex, `ligand_atoms` the ligand's atom indices (1 to N - 1 distinct ones, any
    order); the rest is the receptor, both in ascending complex order.  With E_RL, E_R, E_L the energies of the three systems at
    the complex's positions,

        u = E_RL - E_R - E_L,   E_lam = E_R + E_L + lam u,   F_lam = lam F_RL + (1 - lam) F_(R|L),   dE_lam / dlam = u.

    A binding evaluation reaches the caller's buffers only if all three members' evaluations completed (decided on the device);
    finish() and withheld() report the binding evaluations that are missing.  Do not evaluate or finish a member() directly
    between two finish() calls.

    set_atom_sets(): sets[i] is the set of atom i of the COMPLEX -- its residue, say; a set may mix receptor and ligand atoms.
    Every member gets the restriction to its atoms with the same numbering and the same S; a refused partition leaves the
    earlier one in force."""
    _NEED = "BindingEnergy: the binding has been released"
    _WITHHELD, _DESTROY = "agbnp_hip_binding_withheld_evaluations", "agbnp_hip_binding_destroy"
    _SET_SETS, _NUM_SETS = "agbnp_hip_binding_set_atom_sets", "agbnp_hip_binding_num_atom_sets"
    _OWN_ERRORS = False
    _GROUP = ("binding group", "bindings", _lib.MAX_BINDING_GROUP, True)

    def __init__(self, force, ligand_atoms, device=0, mode="reference"):
        self._h = None
        n = force.getNumParticles()
        lig = _ligand_indices(ligand_atoms, n)  # (before the library is touched)
        mode_bits = HipCalcAGBNPForceKernel.MODES[mode]
        handle = C.c_void_p()
        _check(_lib.load().agbnp_hip_binding_create(C.byref(handle), *_parameters(force), _ip(lig), len(lig), force.getVersion(),
                                                    force.getNonbondedMethod(), force.getCutoffDistance(), device))
        self._h = handle
        self._device = device
        self.numParticles = n
        self._ligand = lig
        self._receptor = np.setdiff1d(np.arange(n, dtype=np.int32), lig).astype(np.int32)
        self._mode = 0
        if mode_bits:
            self.set_mode(mode)

    @property
    def ligand_atoms(self):
        """The ligand's atoms in the ligand context's order (ascending complex order)."""
        return self._ligand.copy()

    @property
    def receptor_atoms(self):
        return self._receptor.copy()

    def execute(self, positions, lam):
        """(E_lam, u, forces[N, 3]) at the complex's positions (N x 3, nm).  Withheld evaluations are repeated inside."""
        pos = self._positions(positions, "execute")
        forces = np.zeros((self.numParticles, 3))
        e, u = C.c_double(0.0), C.c_double(0.0)
        self._call("agbnp_hip_binding_execute_host", _dp(pos), float(lam), _dp(forces), C.byref(e), C.byref(u))
        return e.value, u.value, forces

    def energy(self, positions, lam):
        """(E_lam, u) without forces: three energy-only evaluations.  Withheld evaluations are repeated inside."""
        pos = self._positions(positions, "energy")
        e, u = C.c_double(0.0), C.c_double(0.0)
        self._call("agbnp_hip_binding_energy_host", _dp(pos), float(lam), C.byref(e), C.byref(u))
        return e.value, u.value

    def execute_device(self, d_positions, lam, d_forces, d_energy=None, d_binding_energy=None, stream=None):
        """Raw FP64 device pointers (ints): F_lam is ADDED to d_forces[3N], E_lam to *d_energy, u to *d_binding_energy (either
        may be None) -- all of it or, if any member's evaluation is withheld, nothing.  Asynchronous; call finish()."""
        self._call("agbnp_hip_binding_execute_device", C.c_void_p(d_positions), float(lam), C.c_void_p(d_forces), _ptr(d_energy),
                   _ptr(d_binding_energy), _ptr(stream))

    def energy_device(self, d_positions, lam, d_energy=None, d_binding_energy=None, stream=None):
        """Energy-only form of execute_device(): no force buffer is written; d_energy and d_binding_energy not both None."""
        self._call("agbnp_hip_binding_energy_device", C.c_void_p(d_positions), float(lam), _ptr(d_energy), _ptr(d_binding_energy),
                   _ptr(stream))

    def decompose(self, positions):
        """Per-atom decomposition of the binding energy (include/agbnp_hip.h, agbnp_hip_binding_decompose_host): returns
        (terms, u) with terms a float64 array [4, N] in the order of DECOMPOSITION_TERMS and the complex's atom order,
        terms[t, i] = T_RL[t, i] - T_own[t, own(i)] -- the complex's term of atom i minus the term of the same atom in its own
        sub-system alone -- and terms.sum() = u.  Version 0 has the cavity plane only.  Withheld evaluations are repeated
        inside."""
        pos = self._positions(positions, "decompose")
        terms = np.zeros((len(DECOMPOSITION_TERMS), self.numParticles))
        u = C.c_double(0.0)
        self._call("agbnp_hip_binding_decompose_host", _dp(pos), _dp(terms), C.byref(u))
        return terms, u.value

    def decompose_device(self, d_positions, d_per_atom, d_binding_energy=None, stream=None):
        """Device-resident form of decompose(): the 4 N terms are ADDED to d_per_atom (term-major planes of N doubles) and u to
        *d_binding_energy when it is given -- all of it or, if any member's evaluation is withheld, nothing; raw FP64 device
        pointers (ints).  One binding evaluation in the binding's log; asynchronous, call finish().  Refused (OpenMMException)
        inside a stream capture."""
        self._call("agbnp_hip_binding_decompose_device", C.c_void_p(d_positions), C.c_void_p(d_per_atom), _ptr(d_binding_energy),
                   _ptr(stream))

    def pair_matrix(self, positions):
        """Set-pair matrix of the binding energy (include/agbnp_hip.h, agbnp_hip_binding_pair_matrix_host): returns (D, u) with D
        a float64 array [S, S] over the sets of set_atom_sets(), D = M_RL - M_R - M_L of the members' pair_matrix() tables at the
        complex's positions.  D is symmetric, D.sum() = u, row a sums to the share of set a in decompose()'s terms; for a
        receptor set a and a ligand set b D[a, b] is their direct GB interaction (half of it: D[b, a] is the other half), for
        two receptor sets what the ligand's presence changes between them.  Version 0 fills the diagonal only.  Withheld
        evaluations are repeated inside."""
        pos = self._positions(positions, "pair_matrix")
        s = max(self.num_atom_sets(), 1)  # (no partition: the library refuses, with its message)
        matrix = np.zeros((s, s))
        u = C.c_double(0.0)
        self._call("agbnp_hip_binding_pair_matrix_host", _dp(pos), _dp(matrix), C.byref(u))
        return matrix, u.value

    def pair_matrix_device(self, d_positions, d_matrix, d_binding_energy=None, stream=None):
        """Device-resident form of pair_matrix(): the S S entries of D are ADDED to d_matrix (row-major FP64) and u to
        *d_binding_energy when it is given -- all of it or, if any member's evaluation is withheld, nothing; raw device pointers
        (ints).  One binding evaluation in the binding's log; asynchronous, call finish().  Refused (OpenMMException) inside a
        stream capture and without a partition."""
        self._call("agbnp_hip_binding_pair_matrix_device", C.c_void_p(d_positions), C.c_void_p(d_matrix), _ptr(d_binding_energy),
                   _ptr(stream))

    def finish(self, stream=None):
        """Drains the stream, finishes the three members and returns the number of binding evaluations since the previous
        finish() with at least one withheld member: NOTHING of those reached the caller's buffers; run them again (withheld())."""
        rep = C.c_int(0)
        self._call("agbnp_hip_binding_finish", _ptr(stream), C.byref(rep))
        return int(rep.value)

    def expect_jump(self):
        """The next evaluation's positions are unrelated to the last ones: forwarded to all three members."""
        self._call("agbnp_hip_binding_expect_jump")

    def set_mode(self, mode):
        self._need()
        self._mode = HipCalcAGBNPForceKernel.MODES[mode]
        self._call("agbnp_hip_binding_set_mode", self._mode)

    def copyParametersToContext(self, force):
        """`force` holds the parameters of the COMPLEX; every member gets its subset."""
        self._need()
        self._call("agbnp_hip_binding_update_parameters", *_parameters(force))

    def member(self, which):
        """A HipCalcAGBNPForceKernel view of a member -- 0 or "complex", 1 or "receptor", 2 or "ligand" -- for scalar(), vector(),
        poll() and wait_verdict().  The view does not own the handle: it is valid until release()."""
        self._need()
        which = {"complex": 0, "receptor": 1, "ligand": 2}.get(which, which)
        if which not in (0, 1, 2):
            raise OpenMMException("BindingEnergy.member(): 0 the complex, 1 the receptor, 2 the ligand")
        view = _MemberView(self._device)
        view._h = C.c_void_p(_lib.load().agbnp_hip_binding_member(self._h, which))
        view._mode = self._mode
        view._num_sets = self._num_sets
        view.numParticles = (self.numParticles, len(self._receptor), len(self._ligand))[which]
        return view


class _MemberView(HipCalcAGBNPForceKernel):
    """A member of a BindingEnergy: the binding owns the handle."""

    def initialize(self, force):
        raise OpenMMException("a member of a BindingEnergy is created by the binding")

    def release(self):
        self._h = None


# ---- groups: replica groups of kernels, binding groups of bindings --------------------------------------------------------------
# Each of the fourteen entry points is: the members, checked; what crosses the C ABI, marshalled; one call; the result.
def _members(who, members, cls):
    """The members of a group call as a list, checked: their number, their class, each with a handle, distinct where the
    library demands it (cls._GROUP)."""
    members = list(members)
    kind, noun, bound, distinct = cls._GROUP
    if not 1 <= len(members) <= bound:
        raise OpenMMException(f"{who}(): a {kind} has 1 to {bound} {noun}, not {len(members)}")
    for m in members:
        if not isinstance(m, cls):
            raise OpenMMException(f"{who}(): members must be {cls.__name__} objects")
        m._need()
    if distinct and len({id(m) for m in members}) != len(members):
        raise OpenMMException(f"{who}(): the same binding twice")
    return members


def _pointer_arrays(who, members, optional=False, **lists):
    """The members' handles, then every list of device pointers (ints; None and 0 are NULL), as the ctypes arrays that cross
    the C ABI, one entry per member.  `optional`: a list that is None stays None (every entry NULL)."""
    n = len(members)
    array = C.c_void_p * n
    out = [array(*[m._h for m in members])]
    for name, ptrs in lists.items():
        if ptrs is None and optional:
            out.append(None)
        elif len(ptrs) != n:
            raise OpenMMException(f"{who}(): {name} has {len(ptrs)} entries for {n} {members[0]._GROUP[1]}")
        else:
            out.append(array(*[int(p or 0) for p in ptrs]))
    return out


def _host_arrays(who, members, positions, forces=None, lambdas=None):
    """The host side of a group call, checked: (handles, positions, forces, lambdas).  positions[i] is converted, forces[i]
    must be writable as it is; both cross as arrays of pointers, one per member.  lambdas cross as one float64 array.  What
    is not given comes back as None."""
    n, noun = len(members), members[0]._GROUP[1]
    if forces is None and len(positions) != n:
        raise OpenMMException(f"{who}(): {len(positions)} positions for {n} {noun}")
    if forces is not None and (len(positions) != n or len(forces) != n):
        raise OpenMMException(f"{who}(): {len(positions)} positions and {len(forces)} force arrays for {n} {noun}")
    if lambdas is not None:
        lambdas = np.ascontiguousarray(lambdas, dtype=np.float64).reshape(-1)
        if lambdas.size != n:
            raise OpenMMException(f"{who}(): {lambdas.size} lambdas for {n} {noun}")
        if not np.isfinite(lambdas).all():
            raise OpenMMException(f"{who}(): lambda must be finite")
    pos = [m._positions(p, who) for m, p in zip(members, positions)]
    for m, f in zip(members, () if forces is None else forces):
        _forces_array(f, m.numParticles, f"{who}(): forces must be C-contiguous float64 arrays of 3N values")

    def pointers(arrays):
        out = (C.POINTER(C.c_double) * n)(*[_dp(a) for a in arrays])
        out._arrays = arrays  # (a ctypes array does not keep alive what its entries point to: the converted positions)
        return out
    return _pointer_arrays(who, members)[0], pointers(pos), forces if forces is None else pointers(forces), lambdas


def execute_group(kernels, d_positions, d_forces, d_energies, stream=None):
    """Replica groups (include/agbnp_hip.h, agbnp_hip_execute_group): one call that enqueues an evaluation of every kernel in
    `kernels`, with the launches of the members that can share them made once for all of them.  d_positions, d_forces,
    d_energies: lists of raw FP64 device pointers (ints), one per member; forces and energies are ADDED, as by each member's
    execute_device().  Asynchronous; each member's finish() reports its own withheld evaluations."""
    kernels = _members("execute_group", kernels, HipCalcAGBNPForceKernel)
    hs, pos, frc, ene = _pointer_arrays("execute_group", kernels, d_positions=d_positions, d_forces=d_forces, d_energies=d_energies)
    _check(_lib.load().agbnp_hip_execute_group(hs, len(kernels), pos, frc, ene, _ptr(stream)), kernels[0]._h)


def execute_group_host(kernels, positions, forces):
    """Synchronous twin of execute_group() for host buffers: positions[i] (N_i x 3) are read, forces[i] (C-contiguous float64
    arrays of 3 N_i values) are accumulated in place, the members' energies are returned as a list.  Withheld members are
    repeated inside."""
    kernels = _members("execute_group_host", kernels, HipCalcAGBNPForceKernel)
    hs, pos, frc, _ = _host_arrays("execute_group_host", kernels, positions, forces)
    energies = np.zeros(len(kernels))
    _check(_lib.load().agbnp_hip_execute_group_host(hs, len(kernels), pos, frc, _dp(energies)), kernels[0]._h)
    return [float(e) for e in energies]


def energy_group(kernels, d_positions, d_energies, stream=None):
    """Energy-only replica groups (include/agbnp_hip.h, agbnp_hip_energy_group): one call that enqueues an energy-only
    evaluation of every kernel in `kernels`, with the launches of the members that can share them made once for all of them.
    d_positions, d_energies: lists of raw FP64 device pointers (ints), one per member; position buffers may be shared between
    members, the energy words must be distinct.  The energies are ADDED, as by each member's energy_device(); no force is
    written.  Asynchronous; each member's finish() reports its own withheld evaluations."""
    kernels = _members("energy_group", kernels, HipCalcAGBNPForceKernel)
    hs, pos, ene = _pointer_arrays("energy_group", kernels, d_positions=d_positions, d_energies=d_energies)
    _check(_lib.load().agbnp_hip_energy_group(hs, len(kernels), pos, ene, _ptr(stream)), kernels[0]._h)


def energy_group_host(kernels, positions):
    """Synchronous twin of energy_group() for host buffers: positions[i] (N_i x 3) are read, the members' energies are
    returned as a list.  Withheld members are repeated inside."""
    kernels = _members("energy_group_host", kernels, HipCalcAGBNPForceKernel)
    hs, pos, _, _ = _host_arrays("energy_group_host", kernels, positions)
    energies = np.zeros(len(kernels))
    _check(_lib.load().agbnp_hip_energy_group_host(hs, len(kernels), pos, _dp(energies)), kernels[0]._h)
    return [float(e) for e in energies]


def decompose_group(kernels, d_positions, d_per_atom, d_energies=None, stream=None):
    """Decomposition groups (include/agbnp_hip.h, agbnp_hip_decompose_group): one call that enqueues a per-atom decomposition of
    every kernel in `kernels`, the members that can share on the energy-only group's launches plus ONE plane launch per launch
    set.  d_positions, d_per_atom, d_energies: lists of raw FP64 device pointers (ints), one per member; d_energies may be None
    (no totals).  The planes [4, N_i] and the totals are ADDED, per member gated on its own verdict, as by each member's
    decompose_device(); the members' plane buffers and energy words must not overlap.  Asynchronous; each member's finish()
    reports its own withheld evaluations."""
    kernels = _members("decompose_group", kernels, HipCalcAGBNPForceKernel)
    hs, pos, planes, ene = _pointer_arrays("decompose_group", kernels, True, d_positions=d_positions, d_per_atom=d_per_atom,
                                           d_energies=d_energies)
    if pos is None or planes is None:
        raise OpenMMException("decompose_group(): d_positions and d_per_atom are needed")
    _check(_lib.load().agbnp_hip_decompose_group(hs, len(kernels), pos, planes, ene, _ptr(stream)), kernels[0]._h)


def decompose_group_host(kernels, positions):
    """Synchronous twin of decompose_group() for host buffers: positions[i] (N_i x 3) are read; returns the lists (energies,
    terms) with terms[i] a float64 array [4, N_i] in the order of DECOMPOSITION_TERMS.  Withheld members are repeated inside."""
    kernels = _members("decompose_group_host", kernels, HipCalcAGBNPForceKernel)
    hs, pos, _, _ = _host_arrays("decompose_group_host", kernels, positions)
    terms = [np.zeros((len(DECOMPOSITION_TERMS), k.numParticles)) for k in kernels]
    planes = (C.POINTER(C.c_double) * len(kernels))(*[_dp(t) for t in terms])
    energies = np.zeros(len(kernels))
    _check(_lib.load().agbnp_hip_decompose_group_host(hs, len(kernels), pos, planes, _dp(energies)), kernels[0]._h)
    return [float(e) for e in energies], terms


def _matrix_members(who, kernels):
    """The members of a pair-matrix group, checked, and their S: every member needs a partition set through set_atom_sets()."""
    kernels = _members(who, kernels, HipCalcAGBNPForceKernel)
    for i, k in enumerate(kernels):
        if k._num_sets < 1:
            raise OpenMMException(f"{who}(): member {i}: no partition has been set (set_atom_sets())")
    return kernels, [k._num_sets for k in kernels]


def pair_matrix_group(kernels, d_positions, d_matrices, d_energies=None, stream=None):
    """Pair-matrix groups (include/agbnp_hip.h, agbnp_hip_pair_matrix_group): one call that enqueues a set-pair matrix of every
    kernel in `kernels`, the members that can share on the energy-only group's launches plus ONE matrix launch per launch set.
    d_positions, d_matrices, d_energies: lists of raw FP64 device
    pointers (ints), one per member; d_energies may be None (no totals).  Every member uses its own partition: its matrix
    [S_i, S_i] and its total are ADDED, gated on its own verdict, as by its pair_matrix_device().  Position buffers may be
    shared; the matrices and energy words must not overlap, which is checked here -- like the members' partitions -- before the
    library is reached.  Asynchronous; each member's finish() reports its own withheld evaluations."""
    who = "pair_matrix_group"
    kernels, sizes = _matrix_members(who, kernels)
    hs, pos, mats, ene = _pointer_arrays(who, kernels, True, d_positions=d_positions, d_matrices=d_matrices, d_energies=d_energies)
    if pos is None or mats is None:
        raise OpenMMException(f"{who}(): d_positions and d_matrices are needed")
    # the output spans in bytes: every member's matrix, then (where given) its energy word
    spans = [(int(p or 0), 8 * s * s) for p, s in zip(d_matrices, sizes)]
    spans += [(int(p or 0), 8) for p in (d_energies or ())]
    if any(a == 0 for a, _ in spans) or any(not p for p in d_positions):
        raise OpenMMException(f"{who}(): null pointer")
    for i, (a, na) in enumerate(spans):
        for j, (b, nb) in enumerate(spans[:i]):
            if a < b + nb and b < a + na:
                words = j >= len(kernels)  # (both are energy words: the library's own message for those)
                raise OpenMMException(f"{who}(): " + ("energy words" if words else "matrices") + " of two members overlap")
    _check(_lib.load().agbnp_hip_pair_matrix_group(hs, len(kernels), pos, mats, ene, _ptr(stream)), kernels[0]._h)


def pair_matrix_group_host(kernels, positions):
    """Synchronous twin of pair_matrix_group() for host buffers: positions[i] (N_i x 3) are read; returns the lists (energies,
    matrices) with matrices[i] a float64 array [S_i, S_i] over member i's own partition.  Withheld members are repeated inside."""
    who = "pair_matrix_group_host"
    kernels, sizes = _matrix_members(who, kernels)
    hs, pos, _, _ = _host_arrays(who, kernels, positions)
    matrices = [np.zeros((s, s)) for s in sizes]
    mats = (C.POINTER(C.c_double) * len(kernels))(*[_dp(m) for m in matrices])
    energies = np.zeros(len(kernels))
    _check(_lib.load().agbnp_hip_pair_matrix_group_host(hs, len(kernels), pos, mats, _dp(energies)), kernels[0]._h)
    return [float(e) for e in energies], matrices


def _perturbed_members(who, kernels):
    """The members of a perturbation group, checked, and their M: every member needs sets set through set_parameter_sets()."""
    kernels = _members(who, kernels, HipCalcAGBNPForceKernel)
    for i, k in enumerate(kernels):
        if k._num_parameter_sets < 1:
            raise OpenMMException(f"{who}(): member {i}: no parameter sets have been set (set_parameter_sets())")
    return kernels, [k._num_parameter_sets for k in kernels]


def perturbed_energies_group(kernels, d_positions, d_energies, d_own_energies=None, stream=None):
    """Perturbation groups (include/agbnp_hip.h, agbnp_hip_perturbed_energies_group): one call that enqueues the perturbation
    energies of every kernel in `kernels`, the members that can share on the energy-only group's launches plus ONE perturbation
    launch per launch set.  d_positions, d_energies, d_own_energies: lists of raw FP64 device pointers (ints), one per member;
    d_own_energies may be None.  Every member uses its own sets: its [M_i] energies and its own energy are ADDED, gated on its
    own verdict, as by its perturbed_energies_device().  Position buffers may be shared; the outputs must not overlap.
    Asynchronous; each member's finish() reports its own withheld evaluations."""
    who = "perturbed_energies_group"
    kernels, _ = _perturbed_members(who, kernels)
    hs, pos, ene, own = _pointer_arrays(who, kernels, True, d_positions=d_positions, d_energies=d_energies, d_own_energies=d_own_energies)
    if pos is None or ene is None:
        raise OpenMMException(f"{who}(): d_positions and d_energies are needed")
    _check(_lib.load().agbnp_hip_perturbed_energies_group(hs, len(kernels), pos, ene, own, _ptr(stream)), kernels[0]._h)


def perturbed_energies_group_host(kernels, positions):
    """Synchronous twin of perturbed_energies_group() for host buffers: positions[i] (N_i x 3) are read; returns the lists
    (own energies, energies) with energies[i] a float64 array [M_i] over member i's own sets.  Withheld members are repeated
    inside."""
    who = "perturbed_energies_group_host"
    kernels, _ = _perturbed_members(who, kernels)
    hs, pos, _, _ = _host_arrays(who, kernels, positions)
    energies = [np.zeros(max(k.num_parameter_sets(), 1)) for k in kernels]  # (sized by the library's own count, as perturbed_energies())
    out = (C.POINTER(C.c_double) * len(kernels))(*[_dp(e) for e in energies])
    own = np.zeros(len(kernels))
    _check(_lib.load().agbnp_hip_perturbed_energies_group_host(hs, len(kernels), pos, out, _dp(own)), kernels[0]._h)
    return [float(e) for e in own], energies


def binding_execute_group(bindings, d_positions, d_lambdas, d_forces, d_energies=None, d_binding_energies=None, stream=None):
    """Binding groups (include/agbnp_hip.h, agbnp_hip_binding_execute_group): one call that enqueues an evaluation of every
    BindingEnergy in `bindings` -- one gather launch, the members' evaluations as replica groups, one combine launch.
    d_positions, d_forces, d_energies, d_binding_energies: lists of raw FP64 device pointers (ints), one per binding; entries of
    the last two may be None, and so may the lists.  d_lambdas: ONE raw device pointer to len(bindings) doubles, read by the
    combine launch when it runs -- a kernel enqueued earlier on the stream may have written them.  F_lam, E_lam and u are ADDED,
    per binding all or nothing.  Asynchronous; each binding's finish() reports its own withheld evaluations."""
    bindings = _members("binding_execute_group", bindings, BindingEnergy)
    hs, pos, frc, ene, u = _pointer_arrays("binding_execute_group", bindings, True, d_positions=d_positions, d_forces=d_forces,
                                           d_energies=d_energies, d_binding_energies=d_binding_energies)
    if pos is None or frc is None or not d_lambdas:
        raise OpenMMException("binding_execute_group(): d_positions, d_forces and d_lambdas are needed")
    _check(_lib.load().agbnp_hip_binding_execute_group(hs, len(bindings), pos, C.c_void_p(d_lambdas), frc, ene, u, _ptr(stream)))


def binding_energy_group(bindings, d_positions, d_lambdas, d_energies=None, d_binding_energies=None, stream=None):
    """Energy-only form of binding_execute_group() (agbnp_hip_binding_energy_group): no force buffer is written; of a binding's
    two scalar pointers at least one is given, and they are different words."""
    bindings = _members("binding_energy_group", bindings, BindingEnergy)
    hs, pos, ene, u = _pointer_arrays("binding_energy_group", bindings, True, d_positions=d_positions, d_energies=d_energies,
                                      d_binding_energies=d_binding_energies)
    if pos is None or not d_lambdas:
        raise OpenMMException("binding_energy_group(): d_positions and d_lambdas are needed")
    _check(_lib.load().agbnp_hip_binding_energy_group(hs, len(bindings), pos, C.c_void_p(d_lambdas), ene, u, _ptr(stream)))


def binding_execute_group_host(bindings, positions, lambdas, forces):
    """Synchronous twin of binding_execute_group() for host buffers: positions[k] (N_k x 3) are read, forces[k] (C-contiguous
    float64 arrays of 3 N_k values) are accumulated in place; returns the lists (E_lam, u).  A binding whose evaluation was
    withheld is repeated inside."""
    bindings = _members("binding_execute_group_host", bindings, BindingEnergy)
    hs, pos, frc, lam = _host_arrays("binding_execute_group_host", bindings, positions, forces, lambdas)
    e, u = np.zeros(len(bindings)), np.zeros(len(bindings))
    _check(_lib.load().agbnp_hip_binding_execute_group_host(hs, len(bindings), pos, _dp(lam), frc, _dp(e), _dp(u)))
    return [float(x) for x in e], [float(x) for x in u]


def binding_energy_group_host(bindings, positions, lambdas):
    """Synchronous twin of binding_energy_group() for host buffers: returns the lists (E_lam, u)."""
    bindings = _members("binding_energy_group_host", bindings, BindingEnergy)
    hs, pos, _, lam = _host_arrays("binding_energy_group_host", bindings, positions, lambdas=lambdas)
    e, u = np.zeros(len(bindings)), np.zeros(len(bindings))
    _check(_lib.load().agbnp_hip_binding_energy_group_host(hs, len(bindings), pos, _dp(lam), _dp(e), _dp(u)))
    return [float(x) for x in e], [float(x) for x in u]


def host_tables(radius, ishydrogen):
    """I4 tables from the engine's host code (no device needed)."""
    r = np.ascontiguousarray(radius, dtype=np.float64)
    h = np.ascontiguousarray(ishydrogen, dtype=np.int32)
    n = len(r)
    cap = 64 * 64 * 16
    y, y2 = np.zeros(cap), np.zeros(cap)
    ti, tj = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    ni, nj = C.c_int(0), C.c_int(0)
    _check(_lib.load().agbnp_hip_host_tables(n, _dp(r), _ip(h), C.byref(ni), C.byref(nj), _dp(y), _dp(y2), cap, _ip(ti), _ip(tj)))
    k = ni.value * nj.value * 16
    return dict(y=y[:k].reshape(ni.value, nj.value, 16), y2=y2[:k].reshape(ni.value, nj.value, 16), type_screened=ti,
                type_screener=tj)


class AGBNPContext:
    """Minimal Context + ForceImpl stand-in: positions in, (energy, forces) out, through the kernel."""

    def __init__(self, force, device=0):
        self._force = force
        self._kernel = HipCalcAGBNPForceKernel(device)
        self._kernel.initialize(force)  # AGBNPForceImpl::initialize
        self._positions = None

    @property
    def kernel(self):
        return self._kernel

    def setPositions(self, positions):
        self._positions = np.ascontiguousarray(positions, dtype=np.float64).reshape(-1, 3)

    def _in_groups(self, groups):
        """Whether the force-group mask includes this force (AGBNPForceImpl::calcForcesAndEnergy,
        openmmapi/src/AGBNPForceImpl.cpp:32-36); positions must have been set."""
        if self._positions is None:
            raise OpenMMException("Particle positions have not been set")
        return (groups & (1 << self._force.getForceGroup())) != 0

    def getState(self, groups=-1):
        """Returns (potential energy, forces[N,3]).  Honours the force-group mask like
        AGBNPForceImpl::calcForcesAndEnergy (openmmapi/src/AGBNPForceImpl.cpp:32-36)."""
        forces = np.zeros((self._kernel.numParticles, 3))
        if not self._in_groups(groups):
            return 0.0, forces
        e = self._kernel.execute(self._positions, forces, True, True)
        return e, forces

    def getEnergy(self, groups=-1):
        """The potential energy alone (getState(getEnergy=True) without forces): an energy-only evaluation.  Honours the
        force-group mask like getState()."""
        if not self._in_groups(groups):
            return 0.0
        return self._kernel.energy(self._positions)

    def getEnergyDecomposition(self, groups=-1):
        """(energy, terms[4, N]) at the context's positions: the per-atom terms of DECOMPOSITION_TERMS, which sum to the energy
        (HipCalcAGBNPForceKernel.decompose).  Honours the force-group mask like getState()."""
        if not self._in_groups(groups):
            return 0.0, np.zeros((len(DECOMPOSITION_TERMS), self._kernel.numParticles))
        return self._kernel.decompose(self._positions)

    def getInteractionMatrix(self, sets, groups=-1, num_sets=None):
        """(energy, M[S, S]) at the context's positions for the partition `sets` (one set index per atom): the set-pair
        interaction matrix of HipCalcAGBNPForceKernel.pair_matrix(), whose entries sum to the energy.  Honours the force-group
        mask like getEnergyDecomposition()."""
        inside = self._in_groups(groups)
        self._kernel.set_atom_sets(sets, num_sets)
        if not inside:
            s = self._kernel.num_atom_sets()
            return 0.0, np.zeros((s, s))
        return self._kernel.pair_matrix(self._positions)

    def getPerturbedEnergies(self, gamma, vdw_alpha, charge, groups=-1):
        """(energy, energies[M]) at the context's positions: the context's own energy and the energy under each of the M
        parameter sets gamma, vdw_alpha, charge ([M, N], or [N] for one) -- HipCalcAGBNPForceKernel.perturbed_energies().
        Honours the force-group mask like getEnergyDecomposition()."""
        inside = self._in_groups(groups)
        self._kernel.set_parameter_sets(gamma, vdw_alpha, charge)
        if not inside:
            return 0.0, np.zeros(self._kernel.num_parameter_sets())
        return self._kernel.perturbed_energies(self._positions)

    def _update_parameters(self, force):
        self._kernel.copyParametersToContext(force)
