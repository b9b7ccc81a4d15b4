"""What every Python wrapper hands to the C ABI (include/agbnp_hip.h), pinned without a device and without the library:
`_lib.load` is replaced by an object that records (symbol, arguments) and answers with a settable return code.  For every public
wrapper of AGBNPplugin.py and the direct engine calls of md.py: the call (symbol, argument count, every argument's value and
kind), the failure (exception type, and the message read for the right handle), the refusal (raised before the library is
reached, with its text).

The md drivers are built without their constructors (`object.__new__` plus the attributes the method under test reads, a
stand-in for torch's stream calls), the way `_Fake` of tests/test_replica_group_api.py sets `_h` and `numParticles`: no device
is involved, so all three of their engine calls are covered here rather than left to the GPU suite."""
import contextlib
import ctypes as C
import types

import numpy as np
import pytest

import openmm_agbnp_plugin_amd as P
from openmm_agbnp_plugin_amd import _lib, md

DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int)
NEED_KERNEL = "HipCalcAGBNPForceKernel: initialize() has not been called"
NEED_BINDING = "BindingEnergy: the binding has been released"
CREATED = 0xC0DE  # the handle a recorded create hands out


def address(a):
    """An argument as the integer the callee would see: None, 0 and a NULL pointer are all 0."""
    if a is None:
        return 0
    if isinstance(a, C.c_void_p):
        return a.value or 0
    if isinstance(a, C._Pointer):
        return C.cast(a, C.c_void_p).value or 0
    assert type(a) is int, a
    return a


def message(handle):
    return f"recorded failure for handle {address(handle):#x}"


class Recorder:
    """Stands for both libraries: every agbnp_* attribute is a function that records its call and returns `fail[symbol]` (0)."""

    def __init__(self, record=True):
        self.calls, self.fail, self.record = [], {}, record

    def __getattr__(self, name):
        if not name.startswith("agbnp_"):
            raise AttributeError(name)

        def call(*args):
            if self.record:
                self.calls.append((name, args))
            return self.answer(name, args)
        setattr(self, name, call)
        return call

    def answer(self, name, args):
        if name == "agbnp_hip_last_error":
            return message(args[0]).encode()
        if name.endswith("withheld_evaluations"):  # two evaluations withheld: the second and the fourth
            if args[1] is not None:
                args[1][0], args[1][1] = 1, 3
            return 2
        if name == "agbnp_hip_generation":
            return 7
        if name == "agbnp_hip_num_kernels":
            return 2
        if name == "agbnp_hip_kernel_name":
            return b"kernel%d" % args[0]
        if name == "agbnp_hip_binding_member":
            return 0x7000 + args[1]
        for place, a in enumerate(args):  # output arguments passed with byref
            out = getattr(a, "_obj", None)
            if isinstance(out, C.c_void_p):
                out.value = CREATED
            elif isinstance(out, C.c_double):
                out.value = 10.5 + place
            elif isinstance(out, C.c_int):
                out.value = 2 + place
        return self.fail.get(name, 0)

    def take(self):
        calls, self.calls = self.calls, []
        return calls


@pytest.fixture()
def rec(monkeypatch):
    r = Recorder()
    monkeypatch.setattr(_lib, "load", lambda: r)
    return r


@pytest.fixture()
def no_library(monkeypatch):
    def refuse():
        raise AssertionError("the wrapper reached the library")
    monkeypatch.setattr(_lib, "load", refuse)


@pytest.fixture()
def make():
    """Members with a handle set directly; the handles are taken away again before the real library could see them."""
    made = []

    def kernel(h=0x5000, n=4):
        k = P.HipCalcAGBNPForceKernel()
        k._h, k.numParticles = (C.c_void_p(h) if h else None), n
        made.append(k)
        return k

    def binding(h=0x6000, n=4):
        b = object.__new__(P.BindingEnergy)
        b._h, b.numParticles, b._device, b._mode = (C.c_void_p(h) if h else None), n, 0, 0
        b._ligand, b._receptor = np.array([3], dtype=np.int32), np.array([0, 1, 2], dtype=np.int32)
        made.append(b)
        return b
    yield types.SimpleNamespace(kernel=kernel, binding=binding, kernels=lambda n: [kernel(0x5000 + i) for i in range(n)],
                                bindings=lambda n: [binding(0x6000 + i) for i in range(n)], track=made.append)
    for m in made:
        m._h = None


# ---- what an argument is expected to be ------------------------------------------------------------------------------------------
class Ptr:
    """A raw pointer argument (handle, device pointer, stream): a c_void_p, or NULL given as None."""

    def __init__(self, value):
        self.value = address(value)

    def check(self, a):
        assert a is None or isinstance(a, C.c_void_p), a
        assert address(a) == self.value


class Host:
    """A host array: a typed pointer to the first element of a C-contiguous array of the type; `same`: this very buffer."""

    def __init__(self, ctype, same=None, values=None):
        self.ctype, self.same, self.values = ctype, same, values

    def check(self, a):
        assert isinstance(a, C.POINTER(self.ctype)), a
        backing = getattr(a, "_arr", None)  # (numpy keeps the array alive on the pointer)
        if backing is not None:
            assert backing.flags.c_contiguous and backing.dtype == np.dtype(self.ctype)
            if self.values is not None:
                assert np.array_equal(backing.reshape(-1), np.asarray(self.values).reshape(-1))
        if self.same is not None:
            assert self.same.flags.c_contiguous and self.same.dtype == np.dtype(self.ctype)
            assert address(a) == self.same.ctypes.data


class Out:
    """An output argument passed with byref."""

    def __init__(self, ctype):
        self.ctype = ctype

    def check(self, a):
        assert type(a).__name__ == "CArgObject" and type(a._obj) is self.ctype, a


class PtrList:
    """A ctypes array of raw pointers, one per member; None entries are NULL."""

    def __init__(self, values):
        self.values = [address(v) for v in values]

    def check(self, a):
        assert isinstance(a, C.Array) and a._type_ is C.c_void_p, a
        assert [address(x) for x in a] == self.values


class HostList:
    """A ctypes array of double pointers, one per member, each to the given buffer."""

    def __init__(self, arrays):
        self.arrays = arrays

    def check(self, a):
        assert isinstance(a, C.Array) and a._type_ is DP and len(a) == len(self.arrays), a
        for p, arr in zip(a, self.arrays):
            assert arr.flags.c_contiguous and arr.dtype == np.float64 and address(p) == arr.ctypes.data


class Null:
    def check(self, a):
        assert a is None


def I(value):  # noqa: E743  a count, an index, a flag: a Python int
    return ("int", value)


def F(value):  # a lambda, a cutoff, a timeout: a Python float
    return ("float", value)


def check_call(call, symbol, expected):
    name, args = call
    assert name == symbol
    assert len(args) == len(expected), (name, args)
    for a, want in zip(args, expected):
        if isinstance(want, tuple):
            kind, value = want
            assert type(a).__name__ == kind and a == value, (name, a, want)
        else:
            want.check(a)


def check_one(rec, symbol, expected):
    calls = rec.take()
    assert [c[0] for c in calls] == [symbol]
    check_call(calls[0], symbol, expected)


def fails(rec, symbol, fn, text, exc=P.OpenMMException, code=1):
    """With `symbol` answering a failure, fn() raises `exc` with exactly `text`."""
    rec.fail = {symbol: code}
    with pytest.raises(exc) as info:
        fn()
    assert str(info.value) == text
    rec.fail = {}
    rec.take()


def refused(fn, text, exc=P.OpenMMException):
    with pytest.raises(exc) as info:
        fn()
    assert str(info.value) == text


def force(n=4, version=1):
    f = P.AGBNPForce.from_arrays(np.linspace(0.15, 0.2, n), np.full(n, 49.0), np.full(n, -1.0), np.linspace(-1, 1, n), [0, 1] * (n // 2),
                                 version=version)
    f.setNonbondedMethod(1)
    f.setCutoffDistance(1.5)
    return f


def parameters(f):
    r, g, a, q, h = f._arrays()
    return [Host(C.c_double, same=r), Host(C.c_double, same=g), Host(C.c_double, same=a), Host(C.c_double, same=q), Host(C.c_int, same=h)]


# ---- HipCalcAGBNPForceKernel ----------------------------------------------------------------------------------------------------
def test_kernel_create_and_parameters(rec, make):
    f = force()
    k = P.HipCalcAGBNPForceKernel(device=3, mode="fast")
    make.track(k)
    k.initialize(f)
    create, mode = rec.take()
    check_call(create, "agbnp_hip_create", [Out(C.c_void_p), I(4)] + parameters(f) + [I(1), I(1), F(1.5), I(3)])
    check_call(mode, "agbnp_hip_set_mode", [Ptr(CREATED), I(1)])
    assert address(k._h) == CREATED and k.numParticles == 4
    k.set_mode("fast+single")
    check_one(rec, "agbnp_hip_set_mode", [Ptr(CREATED), I(5)])
    k.copyParametersToContext(f)
    check_one(rec, "agbnp_hip_update_parameters", [Ptr(CREATED), I(4)] + parameters(f))
    fails(rec, "agbnp_hip_set_mode", lambda: k.set_mode("fast"), message(CREATED))
    fails(rec, "agbnp_hip_update_parameters", lambda: k.copyParametersToContext(f), message(CREATED))
    # initialize() again releases the old context first; a failed create is reported for no handle, a failed mode for the new one
    k.initialize(f)
    assert [c[0] for c in rec.calls] == ["agbnp_hip_destroy", "agbnp_hip_create", "agbnp_hip_set_mode"]
    check_call(rec.take()[0], "agbnp_hip_destroy", [Ptr(CREATED)])
    fails(rec, "agbnp_hip_set_mode", lambda: k.initialize(f), message(CREATED))
    fails(rec, "agbnp_hip_create", lambda: k.initialize(f), message(None))
    assert k._h is None
    plain = P.HipCalcAGBNPForceKernel()  # the reference mode sets nothing
    make.track(plain)
    plain.initialize(f)
    assert [c[0] for c in rec.take()] == ["agbnp_hip_create"]
    plain.release()
    check_one(rec, "agbnp_hip_destroy", [Ptr(CREATED)])
    assert plain._h is None
    plain.release()
    assert rec.take() == []


def test_kernel_host_evaluations(rec, make):
    k = make.kernel()
    h = Ptr(k._h)
    pos, frc = np.arange(12.0).reshape(4, 3), np.zeros((4, 3))
    assert k.execute(pos, frc) == 10.5 + 3
    check_one(rec, "agbnp_hip_execute_host", [h, Host(C.c_double, same=pos), Host(C.c_double, same=frc), Out(C.c_double)])
    assert k.energy(pos) == 10.5 + 2
    check_one(rec, "agbnp_hip_energy_host", [h, Host(C.c_double, same=pos), Out(C.c_double)])
    e, terms = k.decompose(pos)
    assert e == 10.5 + 3 and terms.shape == (4, 4) and terms.dtype == np.float64 and not terms.any()
    check_one(rec, "agbnp_hip_decompose_host", [h, Host(C.c_double, same=pos), Host(C.c_double, same=terms), Out(C.c_double)])
    # positions that are not a C-contiguous float64 array are converted, not passed as they are
    for other in (pos.astype(np.float32), np.asfortranarray(pos), pos.tolist()):
        k.energy(other)
        check_one(rec, "agbnp_hip_energy_host", [h, Host(C.c_double, values=pos), Out(C.c_double)])
    msg = message(k._h)
    fails(rec, "agbnp_hip_execute_host", lambda: k.execute(pos, frc), msg)
    fails(rec, "agbnp_hip_energy_host", lambda: k.energy(pos), msg)
    fails(rec, "agbnp_hip_decompose_host", lambda: k.decompose(pos), msg)


def test_kernel_device_evaluations(rec, make):
    k = make.kernel()
    h = Ptr(k._h)
    k.execute_device(11, 22, 33)
    check_one(rec, "agbnp_hip_execute_device", [h, Ptr(11), Ptr(22), Ptr(33), Ptr(0)])
    k.execute_device(11, 22, 33, stream=44)
    check_one(rec, "agbnp_hip_execute_device", [h, Ptr(11), Ptr(22), Ptr(33), Ptr(44)])
    k.execute_device(0, 0, 0, 0)
    check_one(rec, "agbnp_hip_execute_device", [h, Ptr(0), Ptr(0), Ptr(0), Ptr(0)])
    k.energy_device(11, 33)
    check_one(rec, "agbnp_hip_energy_device", [h, Ptr(11), Ptr(33), Ptr(0)])
    k.energy_device(11, 33, 44)
    check_one(rec, "agbnp_hip_energy_device", [h, Ptr(11), Ptr(33), Ptr(44)])
    k.decompose_device(11, 22)
    check_one(rec, "agbnp_hip_decompose_device", [h, Ptr(11), Ptr(22), Ptr(0), Ptr(0)])
    k.decompose_device(11, 22, 33, 44)
    check_one(rec, "agbnp_hip_decompose_device", [h, Ptr(11), Ptr(22), Ptr(33), Ptr(44)])
    k.execute_openmm(11, True, None, 0, 64, 22, None, False)
    check_one(rec, "agbnp_hip_execute_openmm", [h, Ptr(11), I(1), Ptr(0), Ptr(0), I(64), Ptr(22), Ptr(0), I(0), I(0), Ptr(0)])
    k.execute_openmm(11, 0, 12, 13, np.int64(64), 22, 33, 1, energy_slot=5, stream=44)
    check_one(rec, "agbnp_hip_execute_openmm", [h, Ptr(11), I(0), Ptr(12), Ptr(13), I(64), Ptr(22), Ptr(33), I(1), I(5), Ptr(44)])
    k.energy_openmm(11, True, None, None, 64, 33, True)
    check_one(rec, "agbnp_hip_energy_openmm", [h, Ptr(11), I(1), Ptr(0), Ptr(0), I(64), Ptr(33), I(1), I(0), Ptr(0)])
    k.energy_openmm(11, False, 12, 13, 64, 33, False, 5, 44)
    check_one(rec, "agbnp_hip_energy_openmm", [h, Ptr(11), I(0), Ptr(12), Ptr(13), I(64), Ptr(33), I(0), I(5), Ptr(44)])
    msg = message(k._h)
    fails(rec, "agbnp_hip_execute_device", lambda: k.execute_device(11, 22, 33), msg)
    fails(rec, "agbnp_hip_energy_device", lambda: k.energy_device(11, 33), msg)
    fails(rec, "agbnp_hip_decompose_device", lambda: k.decompose_device(11, 22), msg)
    fails(rec, "agbnp_hip_execute_openmm", lambda: k.execute_openmm(11, True, None, 0, 64, 22, None, False), msg)
    fails(rec, "agbnp_hip_energy_openmm", lambda: k.energy_openmm(11, True, None, None, 64, 33, True), msg)


def test_kernel_finish_poll_and_hints(rec, make):
    k = make.kernel()
    h = Ptr(k._h)
    msg = message(k._h)
    assert k.finish() == 2 + 2
    check_one(rec, "agbnp_hip_finish", [h, Ptr(0), Out(C.c_int)])
    k.finish(44)
    check_one(rec, "agbnp_hip_finish", [h, Ptr(44), Out(C.c_int)])
    assert k.poll() == (2 + 1, 2 + 2)
    check_one(rec, "agbnp_hip_poll", [h, Out(C.c_int), Out(C.c_int)])
    assert k.wait_verdict() == (2 + 3, 2 + 4)
    check_one(rec, "agbnp_hip_wait_verdict", [h, I(0), F(10.0), Out(C.c_int), Out(C.c_int)])
    k.wait_verdict(3, timeout=2)
    check_one(rec, "agbnp_hip_wait_verdict", [h, I(3), F(2.0), Out(C.c_int), Out(C.c_int)])
    assert k.withheld() == [1, 3]
    count, fill = rec.take()
    check_call(count, "agbnp_hip_withheld_evaluations", [h, Null(), I(0)])
    check_call(fill, "agbnp_hip_withheld_evaluations", [h, Host(C.c_int), I(2)])
    assert k.generation() == 7
    check_one(rec, "agbnp_hip_generation", [h])
    k.expect_jump()
    check_one(rec, "agbnp_hip_expect_jump", [h])
    k.atom_order_changed()
    check_one(rec, "agbnp_hip_atom_order_changed", [h])
    fails(rec, "agbnp_hip_finish", k.finish, msg)
    fails(rec, "agbnp_hip_expect_jump", k.expect_jump, msg)
    fails(rec, "agbnp_hip_poll", k.poll, "agbnp_hip_poll: no pinned status memory")
    fails(rec, "agbnp_hip_wait_verdict", k.wait_verdict, "agbnp_hip_wait_verdict: no pinned status memory")
    fails(rec, "agbnp_hip_wait_verdict", lambda: k.wait_verdict(0, 2.5),
          "agbnp_hip_wait_verdict: timed out after 2.5 s with 5 evaluation(s) judged", code=_lib.ERR_TIMEOUT)
    rec.fail = {"agbnp_hip_atom_order_changed": 1}  # (its return code is not looked at)
    k.atom_order_changed()
    assert [c[0] for c in rec.take()] == ["agbnp_hip_atom_order_changed"]


def test_kernel_diagnostics(rec, make):
    k = make.kernel()
    h = Ptr(k._h)
    assert k.scalar("variant") == 10.5 + 2
    check_one(rec, "agbnp_hip_get_scalar", [h, I(6), Out(C.c_double)])
    born = k.vector("born")
    assert born.shape == (4,) and born.dtype == np.float64
    check_one(rec, "agbnp_hip_get_vector", [h, I(1), Host(C.c_double, same=born)])
    t = k.tables()
    sizes, tables = rec.take()
    check_call(sizes, "agbnp_hip_get_table_sizes", [h, Out(C.c_int), Out(C.c_int)])
    assert t["y"].shape == t["y2"].shape == (3, 4, 16) and t["type_screened"].dtype == t["type_screener"].dtype == np.int32
    check_call(tables, "agbnp_hip_get_tables", [h, Host(C.c_double, same=t["y"].reshape(-1)), Host(C.c_double, same=t["y2"].reshape(-1)),
                                                Host(C.c_int, same=t["type_screened"]), Host(C.c_int, same=t["type_screener"])])
    k.set_diagnostics(True)
    check_one(rec, "agbnp_hip_set_diagnostics", [h, I(1)])
    k.set_diagnostics(0)
    check_one(rec, "agbnp_hip_set_diagnostics", [h, I(0)])
    k.set_profiling("yes")
    check_one(rec, "agbnp_hip_set_profiling", [h, I(1)])
    assert k.kernel_times() == {"kernel0": (0.0, 0), "kernel1": (0.0, 0)}
    calls = rec.take()
    assert [c[0] for c in calls] == ["agbnp_hip_num_kernels", "agbnp_hip_get_kernel_times", "agbnp_hip_kernel_name", "agbnp_hip_kernel_name"]
    check_call(calls[0], "agbnp_hip_num_kernels", [])
    check_call(calls[1], "agbnp_hip_get_kernel_times", [h, Host(C.c_double), Host(C.c_long)])
    check_call(calls[2], "agbnp_hip_kernel_name", [I(0)])
    check_call(calls[3], "agbnp_hip_kernel_name", [I(1)])
    msg = message(k._h)
    fails(rec, "agbnp_hip_get_scalar", lambda: k.scalar("variant"), msg)
    fails(rec, "agbnp_hip_get_vector", lambda: k.vector("born"), msg)
    for name in ("no such scalar",):
        with pytest.raises(KeyError):
            k.scalar(name)
        with pytest.raises(KeyError):
            k.vector(name)
    assert rec.take() == []


KERNEL_METHODS = dict(
    set_mode=("fast",), execute=(np.zeros((4, 3)), np.zeros((4, 3))), execute_device=(1, 2, 3),
    execute_openmm=(1, True, 0, 0, 64, 2, 3, True), energy=(np.zeros((4, 3)),), energy_device=(1, 3),
    energy_openmm=(1, True, 0, 0, 64, 3, True), decompose=(np.zeros((4, 3)),), decompose_device=(1, 2), atom_order_changed=(),
    expect_jump=(), finish=(), poll=(), wait_verdict=(), withheld=(), generation=(), copyParametersToContext=(None,),
    scalar=("variant",), vector=("born",), tables=(), set_diagnostics=(True,), set_profiling=(True,), kernel_times=())


def test_kernel_refusals_come_before_the_library(no_library, make):
    never = P.HipCalcAGBNPForceKernel()
    for name, args in KERNEL_METHODS.items():
        refused(lambda: getattr(never, name)(*args), NEED_KERNEL)
    never.release()  # (nothing to release: the library is not asked)
    k = make.kernel()
    pos, frc = np.zeros((4, 3)), np.zeros((4, 3))
    refused(lambda: k.execute(np.zeros((5, 3)), frc), "execute(): wrong number of positions")
    refused(lambda: k.energy(np.zeros((5, 3))), "energy(): wrong number of positions")
    refused(lambda: k.decompose(np.zeros(11)), "decompose(): wrong number of positions")
    text = "execute(): forces must be a C-contiguous float64 array of 3N values"
    for bad in (frc.astype(np.float32), np.zeros((3, 4)).T, np.zeros((5, 3)), frc.tolist()):
        refused(lambda: k.execute(pos, bad), text)
    with pytest.raises(KeyError):
        k.set_mode("no such mode")
    with pytest.raises(KeyError):
        P.HipCalcAGBNPForceKernel(mode="no such mode")
    with pytest.raises(AssertionError, match="reached the library"):
        k.execute(pos, frc)


# ---- replica groups ---------------------------------------------------------------------------------------------------------------
def test_replica_group_calls(rec, make):
    ks = make.kernels(4)
    hs = PtrList([k._h for k in ks])
    first = message(ks[0]._h)
    P.execute_group(ks, [1, 2, 3, 4], [5, 6, 7, 8], (9, 10, 11, 12))
    check_one(rec, "agbnp_hip_execute_group", [hs, I(4), PtrList([1, 2, 3, 4]), PtrList([5, 6, 7, 8]), PtrList([9, 10, 11, 12]), Ptr(0)])
    P.execute_group(iter(ks[:2]), [1, None], [0, 6], [9, 10], stream=44)
    check_one(rec, "agbnp_hip_execute_group", [PtrList([k._h for k in ks[:2]]), I(2), PtrList([1, 0]), PtrList([0, 6]), PtrList([9, 10]),
                                               Ptr(44)])
    P.energy_group(ks, [1, 1, 1, 1], [9, 10, 11, 12])
    check_one(rec, "agbnp_hip_energy_group", [hs, I(4), PtrList([1, 1, 1, 1]), PtrList([9, 10, 11, 12]), Ptr(0)])
    P.energy_group(ks[:1], [1], [None], 44)
    check_one(rec, "agbnp_hip_energy_group", [PtrList([ks[0]._h]), I(1), PtrList([1]), PtrList([0]), Ptr(44)])
    fails(rec, "agbnp_hip_execute_group", lambda: P.execute_group(ks, [1, 2, 3, 4], [5, 6, 7, 8], [9, 10, 11, 12]), first)
    fails(rec, "agbnp_hip_energy_group", lambda: P.energy_group(ks, [1, 2, 3, 4], [9, 10, 11, 12]), first)
    # the same kernel twice is the library's to judge
    P.energy_group([ks[0], ks[0]], [1, 2], [3, 4])
    check_one(rec, "agbnp_hip_energy_group", [PtrList([ks[0]._h, ks[0]._h]), I(2), PtrList([1, 2]), PtrList([3, 4]), Ptr(0)])


def test_replica_group_host_calls(rec, make):
    ks = [make.kernel(0x5000, 4), make.kernel(0x5001, 5)]
    hs = PtrList([k._h for k in ks])
    first = message(ks[0]._h)
    pos, frc = [np.ones((4, 3)), np.ones((5, 3))], [np.zeros((4, 3)), np.zeros(15)]
    out = P.execute_group_host(ks, pos, frc)
    assert out == [0.0, 0.0] and all(type(e) is float for e in out)
    check_one(rec, "agbnp_hip_execute_group_host", [hs, I(2), HostList(pos), HostList(frc), Host(C.c_double, values=[0.0, 0.0])])
    assert P.energy_group_host(ks, pos) == [0.0, 0.0]
    check_one(rec, "agbnp_hip_energy_group_host", [hs, I(2), HostList(pos), Host(C.c_double, values=[0.0, 0.0])])
    P.energy_group_host(ks, [pos[0].tolist(), pos[1].astype(np.float32)])  # converted to arrays of their own
    name, args = rec.take()[0]
    for p, given in zip(args[2], pos):
        assert address(p) not in (0, given.ctypes.data)
    fails(rec, "agbnp_hip_execute_group_host", lambda: P.execute_group_host(ks, pos, frc), first)
    fails(rec, "agbnp_hip_energy_group_host", lambda: P.energy_group_host(ks, pos), first)


def test_replica_group_refusals_come_before_the_library(no_library, make):
    ks = [make.kernel(0x5000, 4), make.kernel(0x5001, 5)]
    many = make.kernels(17)
    never = P.HipCalcAGBNPForceKernel()
    pos, frc = [np.zeros((4, 3)), np.zeros((5, 3))], [np.zeros((4, 3)), np.zeros((5, 3))]
    device = dict(execute_group=lambda g, n: P.execute_group(g, [1] * n, [2] * n, [3] * n),
                  energy_group=lambda g, n: P.energy_group(g, [1] * n, [3] * n),
                  execute_group_host=lambda g, n: P.execute_group_host(g, pos[:n], frc[:n]),
                  energy_group_host=lambda g, n: P.energy_group_host(g, pos[:n]))
    for who, call in device.items():
        refused(lambda: call([], 0), f"{who}(): a group has 1 to 16 members, not 0")
        refused(lambda: call(many, 17), f"{who}(): a group has 1 to 16 members, not 17")
        refused(lambda: call([ks[0], "not a kernel"], 2), f"{who}(): members must be HipCalcAGBNPForceKernel objects")
        refused(lambda: call([ks[0], None], 2), f"{who}(): members must be HipCalcAGBNPForceKernel objects")
        refused(lambda: call([never], 1), NEED_KERNEL)
    refused(lambda: P.execute_group(ks, [1, 2], [3], [4, 5]), "execute_group(): d_forces has 1 entries for 2 members")
    refused(lambda: P.execute_group(ks, [1, 2], [3, 4], [5]), "execute_group(): d_energies has 1 entries for 2 members")
    refused(lambda: P.execute_group(ks, [1], [3, 4], [5, 6]), "execute_group(): d_positions has 1 entries for 2 members")
    refused(lambda: P.energy_group(ks, [1], [4, 5]), "energy_group(): d_positions has 1 entries for 2 members")
    refused(lambda: P.energy_group(ks, [1, 2], [5]), "energy_group(): d_energies has 1 entries for 2 members")
    refused(lambda: P.execute_group_host(ks, pos[:1], frc), "execute_group_host(): 1 positions and 2 force arrays for 2 members")
    refused(lambda: P.execute_group_host(ks, pos, frc[:1]), "execute_group_host(): 2 positions and 1 force arrays for 2 members")
    refused(lambda: P.energy_group_host(ks, pos[:1]), "energy_group_host(): 1 positions for 2 members")
    refused(lambda: P.execute_group_host(ks, [pos[1], pos[1]], frc), "execute_group_host(): wrong number of positions")
    refused(lambda: P.energy_group_host(ks, [pos[1], pos[1]]), "energy_group_host(): wrong number of positions")
    text = "execute_group_host(): forces must be C-contiguous float64 arrays of 3N values"
    refused(lambda: P.execute_group_host(ks, pos, [np.zeros((4, 3), dtype=np.float32), frc[1]]), text)
    refused(lambda: P.execute_group_host(ks, pos, [frc[0], np.zeros((3, 5)).T]), text)
    refused(lambda: P.execute_group_host(ks, pos, [frc[0], np.zeros((4, 3))]), text)
    with pytest.raises(AssertionError, match="reached the library"):
        P.execute_group_host(ks, pos, frc)


# ---- BindingEnergy ----------------------------------------------------------------------------------------------------------------
def test_binding_create(rec, make):
    f = force(6)
    b = P.BindingEnergy(f, [4, 1], device=2, mode="fast")
    make.track(b)
    create, mode = rec.take()
    check_call(create, "agbnp_hip_binding_create", [Out(C.c_void_p), I(6)] + parameters(f)
               + [Host(C.c_int, values=[1, 4]), I(2), I(1), I(1), F(1.5), I(2)])
    check_call(mode, "agbnp_hip_binding_set_mode", [Ptr(CREATED), I(1)])
    assert address(b._h) == CREATED and b.numParticles == 6 and b._mode == 1
    assert b.ligand_atoms.tolist() == [1, 4] and b.receptor_atoms.tolist() == [0, 2, 3, 5]
    assert b.ligand_atoms.dtype == b.receptor_atoms.dtype == np.int32
    b.release()
    check_one(rec, "agbnp_hip_binding_destroy", [Ptr(CREATED)])
    assert b._h is None
    plain = P.BindingEnergy(f, [0])
    make.track(plain)
    assert [c[0] for c in rec.take()] == ["agbnp_hip_binding_create"] and plain._mode == 0
    fails(rec, "agbnp_hip_binding_create", lambda: P.BindingEnergy(f, [0]), message(None))

    class Tracked(P.BindingEnergy):  # (a constructor that fails behind the create leaves a handle: taken away with the others)
        def __init__(self, *args, **kwargs):
            make.track(self)
            super().__init__(*args, **kwargs)
    fails(rec, "agbnp_hip_binding_set_mode", lambda: Tracked(f, [0], mode="fast"), message(None))


def test_binding_methods(rec, make):
    b = make.binding()
    h = Ptr(b._h)
    none = message(None)
    pos = np.arange(12.0).reshape(4, 3)
    e, u, frc = b.execute(pos, 0.25)
    assert (e, u) == (10.5 + 4, 10.5 + 5) and frc.shape == (4, 3) and frc.dtype == np.float64 and not frc.any()
    check_one(rec, "agbnp_hip_binding_execute_host", [h, Host(C.c_double, same=pos), F(0.25), Host(C.c_double, same=frc), Out(C.c_double),
                                                      Out(C.c_double)])
    assert b.energy(pos, 1) == (10.5 + 3, 10.5 + 4)
    check_one(rec, "agbnp_hip_binding_energy_host", [h, Host(C.c_double, same=pos), F(1.0), Out(C.c_double), Out(C.c_double)])
    b.execute_device(11, 0.5, 22)
    check_one(rec, "agbnp_hip_binding_execute_device", [h, Ptr(11), F(0.5), Ptr(22), Ptr(0), Ptr(0), Ptr(0)])
    b.execute_device(11, np.float64(0.5), 22, 33, 34, 44)
    check_one(rec, "agbnp_hip_binding_execute_device", [h, Ptr(11), F(0.5), Ptr(22), Ptr(33), Ptr(34), Ptr(44)])
    b.execute_device(0, 0.5, 0)
    check_one(rec, "agbnp_hip_binding_execute_device", [h, Ptr(0), F(0.5), Ptr(0), Ptr(0), Ptr(0), Ptr(0)])
    b.energy_device(11, 0, d_binding_energy=34)
    check_one(rec, "agbnp_hip_binding_energy_device", [h, Ptr(11), F(0.0), Ptr(0), Ptr(34), Ptr(0)])
    b.energy_device(11, 0.5, 33, None, 44)
    check_one(rec, "agbnp_hip_binding_energy_device", [h, Ptr(11), F(0.5), Ptr(33), Ptr(0), Ptr(44)])
    assert b.finish() == 2 + 2
    check_one(rec, "agbnp_hip_binding_finish", [h, Ptr(0), Out(C.c_int)])
    b.finish(44)
    check_one(rec, "agbnp_hip_binding_finish", [h, Ptr(44), Out(C.c_int)])
    assert b.withheld() == [1, 3]
    count, fill = rec.take()
    check_call(count, "agbnp_hip_binding_withheld_evaluations", [h, Null(), I(0)])
    check_call(fill, "agbnp_hip_binding_withheld_evaluations", [h, Host(C.c_int), I(2)])
    b.expect_jump()
    check_one(rec, "agbnp_hip_binding_expect_jump", [h])
    b.set_mode("deterministic")
    check_one(rec, "agbnp_hip_binding_set_mode", [h, I(2)])
    assert b._mode == 2
    f = force()
    b.copyParametersToContext(f)
    check_one(rec, "agbnp_hip_binding_update_parameters", [h, I(4)] + parameters(f))
    for which, code, n in (("complex", 0, 4), (1, 1, 3), ("ligand", 2, 1)):
        view = b.member(which)
        check_one(rec, "agbnp_hip_binding_member", [h, I(code)])
        assert isinstance(view, P.HipCalcAGBNPForceKernel) and address(view._h) == 0x7000 + code
        assert (view.numParticles, view._mode) == (n, 2)
        view.poll()  # a kernel like any other, under the member's handle
        check_one(rec, "agbnp_hip_poll", [Ptr(0x7000 + code), Out(C.c_int), Out(C.c_int)])
        fails(rec, "agbnp_hip_get_scalar", lambda: view.scalar("variant"), message(0x7000 + code))
        refused(lambda: view.initialize(f), "a member of a BindingEnergy is created by the binding")
        view.release()  # the binding owns the handle
        assert view._h is None and rec.take() == []
    fails(rec, "agbnp_hip_binding_execute_host", lambda: b.execute(pos, 0.5), none)
    fails(rec, "agbnp_hip_binding_energy_host", lambda: b.energy(pos, 0.5), none)
    fails(rec, "agbnp_hip_binding_execute_device", lambda: b.execute_device(11, 0.5, 22), none)
    fails(rec, "agbnp_hip_binding_energy_device", lambda: b.energy_device(11, 0.5, 33), none)
    fails(rec, "agbnp_hip_binding_finish", b.finish, none)
    fails(rec, "agbnp_hip_binding_expect_jump", b.expect_jump, none)
    fails(rec, "agbnp_hip_binding_set_mode", lambda: b.set_mode("fast"), none)
    fails(rec, "agbnp_hip_binding_update_parameters", lambda: b.copyParametersToContext(f), none)


BINDING_METHODS = dict(execute=(np.zeros((4, 3)), 0.5), energy=(np.zeros((4, 3)), 0.5), execute_device=(1, 0.5, 2), energy_device=(1, 0.5, 3),
                       finish=(), withheld=(), expect_jump=(), set_mode=("fast",), copyParametersToContext=(None,), member=(0,))


def test_binding_refusals_come_before_the_library(no_library, make):
    gone = make.binding(h=0)
    for name, args in BINDING_METHODS.items():
        refused(lambda: getattr(gone, name)(*args), NEED_BINDING)
    gone.release()
    b = make.binding()
    refused(lambda: b.execute(np.zeros((5, 3)), 0.5), "execute(): wrong number of positions")
    refused(lambda: b.energy(np.zeros((5, 3)), 0.5), "energy(): wrong number of positions")
    refused(lambda: b.member(3), "BindingEnergy.member(): 0 the complex, 1 the receptor, 2 the ligand")
    refused(lambda: b.member("solvent"), "BindingEnergy.member(): 0 the complex, 1 the receptor, 2 the ligand")
    with pytest.raises(KeyError):
        b.set_mode("no such mode")
    f = force(6)
    E = "BindingEnergy(): "
    refused(lambda: P.BindingEnergy(f, []), E + "the ligand has 1 to N - 1 = 5 atoms, not 0")
    refused(lambda: P.BindingEnergy(f, list(range(6))), E + "the ligand has 1 to N - 1 = 5 atoms, not 6")
    refused(lambda: P.BindingEnergy(f, [0, 6]), E + "ligand atom index out of range")
    refused(lambda: P.BindingEnergy(f, [-1]), E + "ligand atom index out of range")
    refused(lambda: P.BindingEnergy(f, [2, 2]), E + "a ligand atom index is given twice")
    refused(lambda: P.BindingEnergy(f, ["x"]), E + "ligand_atoms must be a list of atom indices")
    refused(lambda: P.BindingEnergy(f, None), E + "ligand_atoms must be a list of atom indices")
    with pytest.raises(KeyError):
        P.BindingEnergy(f, [1], mode="no such mode")
    with pytest.raises(AssertionError, match="reached the library"):
        P.BindingEnergy(f, [1])


# ---- binding groups ---------------------------------------------------------------------------------------------------------------
def test_binding_group_calls(rec, make):
    bs = make.bindings(4)
    hs = PtrList([b._h for b in bs])
    none = message(None)
    P.binding_execute_group(bs, [1, 2, 3, 4], 99, [5, 6, 7, 8])
    check_one(rec, "agbnp_hip_binding_execute_group", [hs, I(4), PtrList([1, 2, 3, 4]), Ptr(99), PtrList([5, 6, 7, 8]), Null(), Null(), Ptr(0)])
    P.binding_execute_group(bs, [1, 2, 3, 4], 99, [5, 6, 7, 8], [9, None, 0, 12], (13, 14, 15, 16), stream=44)
    check_one(rec, "agbnp_hip_binding_execute_group", [hs, I(4), PtrList([1, 2, 3, 4]), Ptr(99), PtrList([5, 6, 7, 8]), PtrList([9, 0, 0, 12]),
                                                       PtrList([13, 14, 15, 16]), Ptr(44)])
    P.binding_energy_group(bs, [1, 2, 3, 4], 99, d_binding_energies=[13, 14, 15, 16])
    check_one(rec, "agbnp_hip_binding_energy_group", [hs, I(4), PtrList([1, 2, 3, 4]), Ptr(99), Null(), PtrList([13, 14, 15, 16]), Ptr(0)])
    P.binding_energy_group(iter(bs[:2]), [1, 1], 99, [9, 10], None, 44)
    check_one(rec, "agbnp_hip_binding_energy_group", [PtrList([b._h for b in bs[:2]]), I(2), PtrList([1, 1]), Ptr(99), PtrList([9, 10]), Null(),
                                                      Ptr(44)])
    fails(rec, "agbnp_hip_binding_execute_group", lambda: P.binding_execute_group(bs, [1, 2, 3, 4], 99, [5, 6, 7, 8]), none)
    fails(rec, "agbnp_hip_binding_energy_group", lambda: P.binding_energy_group(bs, [1, 2, 3, 4], 99, [5, 6, 7, 8]), none)


def test_binding_group_host_calls(rec, make):
    bs = [make.binding(0x6000, 4), make.binding(0x6001, 5)]
    hs = PtrList([b._h for b in bs])
    none = message(None)
    pos, frc = [np.ones((4, 3)), np.ones((5, 3))], [np.zeros((4, 3)), np.zeros(15)]
    lam = np.array([0.0, 1.0])
    e, u = P.binding_execute_group_host(bs, pos, lam, frc)
    assert e == u == [0.0, 0.0] and all(type(x) is float for x in e + u)
    check_one(rec, "agbnp_hip_binding_execute_group_host", [hs, I(2), HostList(pos), Host(C.c_double, same=lam), HostList(frc),
                                                            Host(C.c_double, values=[0.0, 0.0]), Host(C.c_double, values=[0.0, 0.0])])
    assert P.binding_energy_group_host(bs, pos, [0.25, 1]) == ([0.0, 0.0], [0.0, 0.0])
    call = rec.take()[0]
    check_call(call, "agbnp_hip_binding_energy_group_host", [hs, I(2), HostList(pos), Host(C.c_double, values=[0.25, 1.0]),
                                                             Host(C.c_double, values=[0.0, 0.0]), Host(C.c_double, values=[0.0, 0.0])])
    assert address(call[1][4]) != address(call[1][5])  # E_lam and u are two arrays
    fails(rec, "agbnp_hip_binding_execute_group_host", lambda: P.binding_execute_group_host(bs, pos, lam, frc), none)
    fails(rec, "agbnp_hip_binding_energy_group_host", lambda: P.binding_energy_group_host(bs, pos, lam), none)


def test_binding_group_refusals_come_before_the_library(no_library, make):
    bs = [make.binding(0x6000, 4), make.binding(0x6001, 5)]
    many = make.bindings(17)
    gone = make.binding(h=0)
    pos, frc = [np.zeros((4, 3)), np.zeros((5, 3))], [np.zeros((4, 3)), np.zeros((5, 3))]
    calls = dict(binding_execute_group=lambda g, n: P.binding_execute_group(g, [1] * n, 99, [2] * n),
                 binding_energy_group=lambda g, n: P.binding_energy_group(g, [1] * n, 99, [2] * n),
                 binding_execute_group_host=lambda g, n: P.binding_execute_group_host(g, pos[:n], [0.5] * n, frc[:n]),
                 binding_energy_group_host=lambda g, n: P.binding_energy_group_host(g, pos[:n], [0.5] * n))
    for who, call in calls.items():
        refused(lambda: call([], 0), f"{who}(): a binding group has 1 to 16 bindings, not 0")
        refused(lambda: call(many, 17), f"{who}(): a binding group has 1 to 16 bindings, not 17")
        refused(lambda: call([bs[0], "not a binding"], 2), f"{who}(): members must be BindingEnergy objects")
        refused(lambda: call([gone], 1), NEED_BINDING)
        refused(lambda: call([bs[0], bs[0]], 2), f"{who}(): the same binding twice")
    X, G, XH, GH = "binding_execute_group(): ", "binding_energy_group(): ", "binding_execute_group_host(): ", "binding_energy_group_host(): "
    refused(lambda: P.binding_execute_group(bs, [1, 2], 99, [3]), X + "d_forces has 1 entries for 2 bindings")
    refused(lambda: P.binding_execute_group(bs, [1], 99, [3, 4]), X + "d_positions has 1 entries for 2 bindings")
    refused(lambda: P.binding_execute_group(bs, [1, 2], 99, [3, 4], [5], None), X + "d_energies has 1 entries for 2 bindings")
    refused(lambda: P.binding_execute_group(bs, [1, 2], 99, [3, 4], None, [5]), X + "d_binding_energies has 1 entries for 2 bindings")
    refused(lambda: P.binding_energy_group(bs, [1, 2], 99, [5, 6], [7]), G + "d_binding_energies has 1 entries for 2 bindings")
    for missing in (None, 0):
        refused(lambda: P.binding_execute_group(bs, [1, 2], missing, [3, 4]), X + "d_positions, d_forces and d_lambdas are needed")
        refused(lambda: P.binding_energy_group(bs, [1, 2], missing, [3, 4]), G + "d_positions and d_lambdas are needed")
    refused(lambda: P.binding_execute_group(bs, None, 99, [3, 4]), X + "d_positions, d_forces and d_lambdas are needed")
    refused(lambda: P.binding_execute_group(bs, [1, 2], 99, None), X + "d_positions, d_forces and d_lambdas are needed")
    refused(lambda: P.binding_energy_group(bs, None, 99, [3, 4]), G + "d_positions and d_lambdas are needed")
    refused(lambda: P.binding_execute_group_host(bs, pos[:1], [0.0, 1.0], frc), XH + "1 positions and 2 force arrays for 2 bindings")
    refused(lambda: P.binding_energy_group_host(bs, pos[:1], [0.0, 1.0]), GH + "1 positions for 2 bindings")
    refused(lambda: P.binding_execute_group_host(bs, pos, [0.0], frc), XH + "1 lambdas for 2 bindings")
    refused(lambda: P.binding_energy_group_host(bs, pos, [0.0, 0.5, 1.0]), GH + "3 lambdas for 2 bindings")
    for bad in (float("nan"), float("inf")):
        refused(lambda: P.binding_execute_group_host(bs, pos, [0.0, bad], frc), XH + "lambda must be finite")
        refused(lambda: P.binding_energy_group_host(bs, pos, [bad, 1.0]), GH + "lambda must be finite")
    refused(lambda: P.binding_execute_group_host(bs, [pos[1], pos[1]], [0.0, 1.0], frc), XH + "wrong number of positions")
    refused(lambda: P.binding_energy_group_host(bs, [pos[1], pos[1]], [0.0, 1.0]), GH + "wrong number of positions")
    text = XH + "forces must be C-contiguous float64 arrays of 3N values"
    refused(lambda: P.binding_execute_group_host(bs, pos, [0.0, 1.0], [frc[0], np.zeros((5, 3), dtype=np.float32)]), text)
    refused(lambda: P.binding_execute_group_host(bs, pos, [0.0, 1.0], [np.zeros((3, 4)).T, frc[1]]), text)
    with pytest.raises(AssertionError, match="reached the library"):
        P.binding_execute_group(bs, [1, 2], 99, [3, 4], [5, None], None)
    with pytest.raises(AssertionError, match="reached the library"):
        P.binding_energy_group_host(bs, pos, [0.0, 1.0])


# ---- host tables, the context stand-in --------------------------------------------------------------------------------------------
def test_host_tables(rec):
    radius, ish = [0.15, 0.17, 0.12], [0, 0, 1]
    t = P.host_tables(radius, ish)
    name, args = rec.calls[0]
    check_one(rec, "agbnp_hip_host_tables", [I(3), Host(C.c_double, values=radius), Host(C.c_int, values=ish), Out(C.c_int), Out(C.c_int),
                                             Host(C.c_double), Host(C.c_double), I(64 * 64 * 16), Host(C.c_int, same=t["type_screened"]),
                                             Host(C.c_int, same=t["type_screener"])])
    assert t["y"].shape == t["y2"].shape == (5, 6, 16)  # the sizes the call wrote
    assert address(args[5]) == t["y"].ctypes.data and address(args[6]) == t["y2"].ctypes.data
    fails(rec, "agbnp_hip_host_tables", lambda: P.host_tables(radius, ish), message(None))


def test_the_context_guards_its_force_group(rec, make):
    f = force()
    ctx = P.AGBNPContext(f, device=1)
    make.track(ctx.kernel)
    check_call(rec.take()[0], "agbnp_hip_create", [Out(C.c_void_p), I(4)] + parameters(f) + [I(1), I(1), F(1.5), I(1)])
    for get in (ctx.getState, ctx.getEnergy, ctx.getEnergyDecomposition):
        refused(get, "Particle positions have not been set")
    ctx.setPositions(np.arange(12.0))
    f.setForceGroup(3)
    e, frc = ctx.getState(groups=1 << 2)
    assert e == 0.0 and frc.shape == (4, 3) and not frc.any()
    assert ctx.getEnergy(groups=0) == 0.0
    e, terms = ctx.getEnergyDecomposition(groups=7)
    assert e == 0.0 and terms.shape == (4, 4) and not terms.any()
    assert rec.take() == []  # a masked group evaluates nothing
    ctx.getState(groups=1 << 3)
    ctx.getEnergy()
    ctx.getEnergyDecomposition(-1)
    assert [c[0] for c in rec.take()] == ["agbnp_hip_execute_host", "agbnp_hip_energy_host", "agbnp_hip_decompose_host"]
    f.updateParametersInContext(ctx)
    check_one(rec, "agbnp_hip_update_parameters", [Ptr(CREATED), I(4)] + parameters(f))


def test_the_parameter_arrays_follow_the_force():
    f = P.AGBNPForce()
    assert f.addParticle(0.15, 1.0, -1.0, 0.5, False) == 0 and f.addParticle(0.12, 2.0, -2.0, -0.5, True) == 1
    f.setParticleParameters(0, 0.16, 1.5, -1.5, 0.25, True)  # before the arrays exist
    arrays = f._arrays()
    assert [a.tolist() for a in arrays] == [[0.16, 0.12], [1.5, 2.0], [-1.5, -2.0], [0.25, -0.5], [1, 1]]
    assert [a.dtype for a in arrays] == [np.float64] * 4 + [np.int32]
    f.setParticleParameters(1, 0.13, 3.0, -3.0, 0.0, False)  # in place: the same arrays cross the boundary again
    assert f._arrays() is arrays and [a[1] for a in arrays] == [0.13, 3.0, -3.0, 0.0, 0]
    assert f.getParticleParameters(1) == (0.13, 3.0, -3.0, 0.0, False)
    f.addParticle(0.2, 1.0, -1.0, 0.0, False)  # a new particle: new arrays
    assert f._arrays() is not arrays and len(f._arrays()[0]) == 3


# ---- md.py's direct engine calls --------------------------------------------------------------------------------------------------
def _array(values):
    return (C.c_void_p * len(values))(*values)


def _group_md(cls, members):
    g = object.__new__(cls)
    g.kernels, g.R = members, len(members)
    g._handles = _array([m._h for m in members])
    g._pos, g._frc, g._ene = _array([1, 2]), _array([3, 4]), _array([5, 6])
    return g


def test_md_group_evaluation(rec, make):
    ks = make.kernels(2)
    g = _group_md(md._GroupMD, ks)
    g._evaluate(44)
    check_one(rec, "agbnp_hip_execute_group", [PtrList([k._h for k in ks]), I(2), PtrList([1, 2]), PtrList([3, 4]), PtrList([5, 6]), Ptr(44)])
    g._evaluate(0)
    name, args = rec.take()[0]
    assert args[0] is g._handles and args[2] is g._pos and args[3] is g._frc and args[4] is g._ene  # the prebuilt arrays
    Ptr(0).check(args[5])
    fails(rec, "agbnp_hip_execute_group", lambda: g._evaluate(44), "agbnp_hip_execute_group: " + message(ks[0]._h), exc=RuntimeError)


def test_md_binding_evaluation(rec, make):
    bs = make.bindings(2)
    g = _group_md(md.BindingReplicaMD, bs)
    g.lam = types.SimpleNamespace(data_ptr=lambda: 99)
    g._u = _array([7, 8])
    head = [PtrList([b._h for b in bs]), I(2), PtrList([1, 2]), Ptr(99), PtrList([3, 4]), PtrList([5, 6])]
    g._chunk(2, True)  # two evaluations, an attempt behind them: the second one alone passes the u pointers
    g._evaluate(44)
    check_one(rec, "agbnp_hip_binding_execute_group", head + [Null(), Ptr(44)])
    g._evaluate(44)
    check_one(rec, "agbnp_hip_binding_execute_group", head + [PtrList([7, 8]), Ptr(44)])
    g._evaluate(44)
    check_one(rec, "agbnp_hip_binding_execute_group", head + [Null(), Ptr(44)])
    g._chunk(1, False)
    g._evaluate(0)
    check_one(rec, "agbnp_hip_binding_execute_group", head + [Null(), Ptr(0)])
    fails(rec, "agbnp_hip_binding_execute_group", lambda: g._evaluate(44), "agbnp_hip_binding_execute_group: " + message(None), exc=RuntimeError)


class _Stream:
    cuda_stream = 44

    def wait_stream(self, other):
        pass


_TORCH = types.SimpleNamespace(cuda=types.SimpleNamespace(current_stream=lambda: None, stream=lambda s: contextlib.nullcontext()))


def test_md_hamiltonian_exchange(rec, make):
    ks = make.kernels(3)
    h = object.__new__(md.HamiltonianReplicaMD)
    h.torch, h.stream, h.kernels, h._attempt = _TORCH, _Stream(), ks, 0
    h.attempts = types.SimpleNamespace(add_=lambda n: rec.calls.append(("attempts.add_", (n,))))
    h.core = types.SimpleNamespace(lib=rec, part_read=1, forces=lambda torch, st, evaluate: rec.calls.append(("core.forces", (st, evaluate))))
    h._h = (md._HamiltonianArgs(), md._HamiltonianArgs())
    members = [1, 2]
    handles, pos, ene = _array([ks[1]._h, ks[2]._h]), _array([12, 11]), _array([21, 22])
    h._cross_round = [([], _array([None]), _array([None]), _array([None])), (members, handles, pos, ene)]
    h.exchange()  # the even attempt of this ladder has no pair: it only counts
    assert rec.take() == [("attempts.add_", (1,))]
    h.exchange()
    calls = rec.take()
    assert [c[0] for c in calls] == ["agbnp_hip_expect_jump"] * 2 + ["agbnp_hip_energy_group", "agbnp_md_hamiltonian_exchange"] \
        + ["agbnp_hip_expect_jump"] * 2 + ["core.forces"]
    for call, k in zip(calls[:2] + calls[4:6], [ks[1], ks[2]] * 2):
        check_call(call, "agbnp_hip_expect_jump", [Ptr(k._h)])
    check_call(calls[2], "agbnp_hip_energy_group", [PtrList([ks[1]._h, ks[2]._h]), I(2), PtrList([12, 11]), PtrList([21, 22]), Ptr(44)])
    assert calls[2][1][0] is handles and calls[2][1][2] is pos and calls[2][1][3] is ene
    assert calls[3][1][0]._obj is h._h[1] and calls[3][1][1] == 44  # the struct of the partial buffer last read
    assert calls[6][1][0] == 44 and calls[6][1][1] == h._evaluate
    h._attempt = 1
    fails(rec, "agbnp_hip_energy_group", h.exchange, "agbnp_hip_energy_group: " + message(ks[1]._h), exc=RuntimeError)
    h._attempt = 1
    fails(rec, "agbnp_md_hamiltonian_exchange", h.exchange, "libagbnp_md.so: launch failed (hipError 700)", exc=RuntimeError, code=700)
