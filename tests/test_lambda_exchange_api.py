"""Binding groups and the lambda exchange (include/agbnp_hip.h: agbnp_hip_binding_execute_group and its kin; csrc/md_kernels.hip:
agbnp_md_lambda_exchange; md.py: BindingReplicaMD) at the boundaries that need no device: the restatement of the
launch (tests/lambda_exchange_restatement.py) against itself, Delta against the Hamiltonian it stands for, the struct and record
layouts against the kernel file's text, the prototypes, and the checks the Python layers make before they touch a library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import AGBNPplugin as TOP
import openmm_agbnp_plugin_amd as P
from openmm_agbnp_plugin_amd import _lib, md
from tests import lambda_exchange_restatement as lr
from tests import md_restatement as mr
from tests.binding_restatement import BindingRestatement, combine
from tests.test_replica_md_api import _System, no_library  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUP = ("agbnp_hip_binding_execute_group", "agbnp_hip_binding_energy_group", "agbnp_hip_binding_execute_group_host",
         "agbnp_hip_binding_energy_group_host")


# ---- the restatement against itself ------------------------------------------------------------------------------------------
def _run(R, attempts=lr.ATTEMPTS, counter_word=lr.LAMBDA_WORD, **kw):
    state = lr.lambda_state(R, attempts=attempts, **kw)
    states = []
    for i in range(attempts):
        before = lr.energies(state, i)
        state = lr.exchange(before, lr.EXCHANGE_SEED, counter_word=counter_word)
        states.append((before, state))
    return states


@pytest.mark.parametrize("R", lr.SIZES)
def test_the_maps_stay_inverse_and_every_rung_keeps_its_lambda(R):
    """After any number of attempts the maps are inverse permutations, lambda[replica_at_rung[k]] is the ladder's lambda_k bit for
    bit, the baths and steps have not moved, all R u words are zero and every tail is what it was."""
    ladder = lr.ladder(R)
    for i, (before, after) in enumerate(_run(R)):
        at, of = after["replica_at_rung"][:R], after["rung_of_replica"][:R]
        assert sorted(at) == list(range(R)) and np.array_equal(of[at], np.arange(R))
        assert after["lambda"][:R][at].tobytes() == ladder.tobytes()
        a = int(before["attempts"][0])
        assert a == lr.FIRST_ATTEMPT + i and int(after["attempts"][0]) == a + 1
        busy = {int(before["replica_at_rung"][k]) for pair in lr.pairs(a, R) for k in pair}
        assert all(np.isnan(before["u"][r]) for r in set(range(R)) - busy)  # (sentinels where no pair reads)
        assert after["u"][:R].tobytes() == np.zeros(R).tobytes()  # all R words, read or not
        assert after["u"][R:].tobytes() == before["u"][R:].tobytes()
        for key in ("kT", "step"):
            assert after[key].tobytes() == before[key].tobytes()
        for key in ("lambda", "rung_of_replica", "replica_at_rung"):
            assert after[key][R:].tobytes() == before[key][R:].tobytes()
        assert after["attempts"][1:].tobytes() == before["attempts"][1:].tobytes()


@pytest.mark.parametrize("R", lr.SIZES)
def test_record_places_follow_exchange_places(R):
    states = _run(R)
    final = states[-1][1]
    total = md.exchange_places(lr.FIRST_ATTEMPT + lr.ATTEMPTS, R) - md.exchange_places(lr.FIRST_ATTEMPT, R)
    assert len(final["records"]) == max(total, 1)
    if R == 1:
        assert set(final["records"].tobytes()) == {0xFF}
        return
    place = 0
    for before, after in states:
        a = int(before["attempts"][0])
        assert place == md.exchange_places(a, R) - before["record_base"] == mr.exchange_places(a, R) - before["record_base"]
        for t, (k, k1) in enumerate(lr.pairs(a, R)):
            rec = after["records"][place + t]
            lo, hi = int(before["replica_at_rung"][k]), int(before["replica_at_rung"][k1])
            assert (rec["attempt"], rec["rung"], rec["replica_lo"], rec["replica_hi"]) == (a, k, lo, hi)
            assert rec["step"] == 1000 + 7 * lo
            for key, want in (("u_lo", before["u"][lo]), ("u_hi", before["u"][hi]), ("lambda_lo", before["lambda"][lo]),
                              ("lambda_hi", before["lambda"][hi]), ("kT_lo", before["kT"][lo]), ("kT_hi", before["kT"][hi])):
                assert rec[key].tobytes() == np.float64(want).tobytes(), key  # everything BEFORE the decision
            assert rec["uniform"] == md.lambda_uniform(k, a, lr.EXCHANGE_SEED)
            assert set(after["records"][place + len(lr.pairs(a, R)):].tobytes()) <= {0xFF}
        place += len(lr.pairs(a, R))
    assert place == total


def test_with_word_two_the_deviates_are_the_temperature_exchanges():
    for R in (2, 3, 16):
        for before, after in _run(R, counter_word=lr.TEMPERATURE_WORD):
            a = int(before["attempts"][0])
            first = md.exchange_places(a, R) - before["record_base"]
            for t, (k, _) in enumerate(lr.pairs(a, R)):
                assert after["records"][first + t]["uniform"] == md.exchange_uniform(k, a, lr.EXCHANGE_SEED)
    w = md.philox4x32((3, 7, 1, 4), (0x12345678, 0x9))
    assert md.lambda_uniform(3, (1 << 32) + 7, (0x9 << 32) | 0x12345678) == md.uniform53(w[0], w[1])
    assert md.lambda_uniform(3, 9, 5) not in (md.exchange_uniform(3, 9, 5), md.hamiltonian_uniform(3, 9, 5))
    assert (md.PHILOX_EXCHANGE, md.PHILOX_HAMILTONIAN, md.PHILOX_LAMBDA) == (2, 3, 4)


def test_no_verdict_of_the_gpu_tests_inputs_lies_in_the_band():
    """The inputs of tests/test_gpu_lambda_exchange_kernel.py judged by the restatement alone: every record's |log(uniform) -
    Delta| / max(1, |Delta|) is far above the 1e-9 band, so the GPU test compares EVERY verdict; both verdicts occur at every
    R > 1."""
    for R in lr.SIZES:
        smallest, verdicts = np.inf, []
        for _, after in _run(R):
            pass
        total = md.exchange_places(lr.FIRST_ATTEMPT + lr.ATTEMPTS, R) - md.exchange_places(lr.FIRST_ATTEMPT, R)
        for rec in (after["records"][:total] if R > 1 else []):
            m, d = lr.margin(rec)
            smallest = min(smallest, m)
            verdicts.append(int(rec["accepted"]))
            assert rec["accepted"] == int(np.log(np.longdouble(rec["uniform"])) <= d)
        if R > 1:
            assert smallest > 1e-6 > lr.BAND, f"R {R}: a verdict hangs on {smallest:.2e}"
            assert set(verdicts) == {0, 1}, f"R {R}: verdicts {set(verdicts)}"
            print(f"R {R}: smallest margin {smallest:.2e}, {sum(verdicts)} of {len(verdicts)} accepted")
    # the truncated log of the GPU test: the same decisions
    full, cut = _run(16)[-1][1], _run(16, log_capacity=12)[-1][1]
    assert cut["records"][:12].tobytes() == full["records"][:12].tobytes() and set(cut["records"][12:].tobytes()) == {0xFF}
    assert np.array_equal(cut["replica_at_rung"], full["replica_at_rung"]) and cut["lambda"].tobytes() == full["lambda"].tobytes()


def test_the_crafted_pairs_are_what_they_say():
    """Delta = +50 and -50 give certain verdicts; a u word that is 0.0, -0.0, NaN or infinite makes the pair void: recorded with
    accepted = -1, nothing swapped, the two u words handed back as zeros all the same."""
    before = lr.crafted_state()
    after = lr.exchange(before, lr.EXCHANGE_SEED)
    recs = after["records"]
    assert len(recs) == 8 and list(recs["accepted"][:6]) == [1, 0, -1, -1, -1, -1]
    deltas = [float(lr.margin(rec)[1]) for rec in recs[:2]]
    assert abs(deltas[0] - 50.0) < 1e-9 and abs(deltas[1] + 50.0) < 1e-9
    assert abs(md.lambda_delta(*(recs[0][key] for key in ("lambda_lo", "lambda_hi", "kT_lo", "kT_hi", "u_lo", "u_hi"))) - 50.0) < 1e-9
    assert all(lr.margin(rec)[0] > 1e-6 for rec in list(recs[:2]) + list(recs[6:]))
    assert recs["u_lo"][2] == 0.0 and np.signbit(recs["u_lo"][3]) and np.isnan(recs["u_hi"][4]) and np.isinf(recs["u_hi"][5])
    assert list(after["replica_at_rung"][:12]) == [1, 0] + list(range(2, 12))
    assert after["lambda"][0] == before["lambda"][1] and after["lambda"][1] == before["lambda"][0]
    assert after["lambda"][2:16].tobytes() == before["lambda"][2:16].tobytes() or recs["accepted"][6:].any()
    assert after["lambda"][4:12].tobytes() == before["lambda"][4:12].tobytes()  # the void pairs
    assert after["u"][:16].tobytes() == np.zeros(16).tobytes()


# ---- Delta is the Hamiltonian's ----------------------------------------------------------------------------------------------
def test_delta_is_the_change_of_the_reduced_hamiltonians(systems):
    """Two trpcage geometries (ligand 0 .. 15, jitter steps 0 and 1) at lambda = 0.25 / 0.5 and two baths: Delta from u alone
    equals -[E_hi(x_lo)/kT_lo + E_lo(x_hi)/kT_hi - E_lo(x_lo)/kT_lo - E_hi(x_hi)/kT_hi], the four E_lambda formed by the binding
    restatement in long double (the right-hand side cancels E_R + E_L, thousands of kT, to a Delta of order 0.1).  The two
    agree to 1e-9 relative."""
    s = systems("trpcage")
    ligand = range(16)
    ref = BindingRestatement(s.params(), ligand)
    x = [s.jittered(0), s.jittered(1)]
    evals = [ref.evaluate(p) for p in x]
    u = [combine(*e, 0.0)[1] for e in evals]
    print("u (kJ/mol):", u)
    for kT in ((md.KB * 300.0, md.KB * 300.0), (md.KB * 300.0, md.KB * 330.0)):
        for l_lo, l_hi in ((0.25, 0.5), (0.5, 0.25)):
            def e(lam, j):  # E_lambda(x_j) by combine()'s formula, from the restatement's three energies
                e_rl, e_r, e_l = (np.longdouble(w) for w in evals[j][0])
                assert float((1 - np.longdouble(lam)) * (e_r + e_l) + np.longdouble(lam) * e_rl) == pytest.approx(combine(*evals[j], lam)[0], rel=1e-14)
                return (1 - np.longdouble(lam)) * (e_r + e_l) + np.longdouble(lam) * e_rl

            terms = [e(l_hi, 0) / kT[0], e(l_lo, 1) / kT[1], e(l_lo, 0) / kT[0], e(l_hi, 1) / kT[1]]
            rhs = float(-(terms[0] + terms[1] - terms[2] - terms[3]))
            delta = md.lambda_delta(l_lo, l_hi, kT[0], kT[1], u[0], u[1])
            assert float(lr.delta_of(l_lo, l_hi, kT[0], kT[1], u[0], u[1])) == pytest.approx(delta, rel=1e-12, abs=1e-12)
            scale = max(abs(t) for t in terms)
            print(f"lambda {l_lo} / {l_hi}, kT {kT}: Delta {delta:.9f}, from the four energies {rhs:.9f}, terms up to {float(scale):.3e}")
            assert abs(delta - rhs) <= 1e-9 * abs(delta)
            assert 0.01 < abs(delta) < 5.0
    assert md.lambda_delta(0.25, 0.5, 2.5, 2.5, 444.0, 442.0) == -md.lambda_delta(0.5, 0.25, 2.5, 2.5, 444.0, 442.0)
    assert md.lambda_delta(0.25, 0.25, 2.5, 2.6, 444.0, 442.0) == 0.0


# ---- layouts and prototypes --------------------------------------------------------------------------------------------------
def _struct_fields(text, name):
    """(type, name) of every member of `struct name { ... };` in the kernel file, comments dropped, in order."""
    body = re.search(r"struct %s \{[^\n]*\n(.*?)\n\};" % name, text, re.S).group(1)
    fields = []
    for line in body.split("\n"):
        line = line.split("//")[0].strip().rstrip(";")
        if not line:
            continue
        pointer_type = "*" in line
        names = [w.strip() for w in re.sub(r"^(const )?(unsigned )?(long long|double|int|\w+)\s*\**", "", line).split(",")]
        for w in names:
            fields.append(("pointer" if pointer_type or w.startswith("*") else line.split()[0], w.lstrip("* ")))
    return fields


def test_the_struct_and_the_record_have_the_kernels_layout():
    text = open(os.path.join(ROOT, "openmm_agbnp_plugin_amd", "csrc", "md_kernels.hip")).read()
    assert "struct AgbnpMdLambda {  // (md.py::_LambdaArgs)" in text and "struct AgbnpMdLambdaRecord {  // (md.py::LAMBDA_RECORD); 88 bytes" in text
    fields = _struct_fields(text, "AgbnpMdLambda")
    assert [name for _, name in fields] == [name for name, _ in md._LambdaArgs._fields_]
    assert fields[0][0] == "int" and all(kind in ("pointer", "long", "unsigned") for kind, _ in fields[1:])
    assert C.sizeof(md._LambdaArgs) == 8 + 10 * 8 and md._LambdaArgs.replicas.offset == 0
    assert [getattr(md._LambdaArgs, name).offset for name, _ in md._LambdaArgs._fields_[1:]] == [8 + 8 * j for j in range(10)]
    rec = md.LAMBDA_RECORD
    assert rec.itemsize == 88 == 2 * 8 + 4 * 4 + 7 * 8
    assert rec.names == ("attempt", "step", "rung", "replica_lo", "replica_hi", "accepted", "u_lo", "u_hi", "lambda_lo", "lambda_hi",
                         "kT_lo", "kT_hi", "uniform")
    assert [name for _, name in _struct_fields(text, "AgbnpMdLambdaRecord")] == list(rec.names)
    assert [rec.fields[name][1] for name in rec.names] == [0, 8, 16, 20, 24, 28] + [32 + 8 * j for j in range(7)]
    assert md.LAMBDA_SYMBOLS == ("agbnp_md_lambda_exchange",)
    assert "int agbnp_md_lambda_exchange(const AgbnpMdLambda* e, void* stream)" in text and "kLambdaWord = 4u" in text
    lib = C.CDLL(os.path.join(ROOT, "openmm_agbnp_plugin_amd", "libagbnp_md.so"))
    lib.agbnp_md_lambda_exchange.argtypes = [C.c_void_p, C.c_void_p]
    assert lib.agbnp_md_lambda_exchange(None, None) != 0  # (refused on the host: no device is touched)
    bad = md._LambdaArgs(replicas=17)
    assert lib.agbnp_md_lambda_exchange(C.byref(bad), None) != 0
    assert "asm" not in text


def test_the_group_entry_points_are_declared_and_exported():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "agbnp_hip.h")).read()
    for name in GROUP:
        assert name in _lib.SYMBOLS and f"int {name}(agbnp_hip_binding* const* bindings, int count," in header
        getattr(lib, name)
    m = re.search(r"#define AGBNP_HIP_MAX_BINDING_GROUP (\d+)", header)
    assert m and int(m.group(1)) == _lib.MAX_BINDING_GROUP == 16
    assert "const double* d_lambdas" in header
    for name in ("binding_execute_group", "binding_energy_group", "binding_execute_group_host", "binding_energy_group_host"):
        assert getattr(TOP, name) is getattr(P, name)
    bad = _lib.ERR_INVALID_ARGUMENT
    assert lib.agbnp_hip_binding_execute_group(None, 1, None, None, None, None, None, None) == bad
    assert lib.agbnp_hip_binding_energy_group(None, 1, None, None, None, None, None) == bad
    assert lib.agbnp_hip_binding_execute_group_host(None, 1, None, None, None, None, None) == bad
    assert lib.agbnp_hip_binding_energy_group_host(None, 1, None, None, None, None) == bad
    handles = (C.c_void_p * 17)()  # counts are judged before the bindings are looked at
    for count in (0, 17, -1):
        assert lib.agbnp_hip_binding_execute_group(handles, count, None, None, None, None, None, None) == bad
        assert "1 to 16" in _lib.last_error(None)
    assert lib.agbnp_hip_binding_execute_group(handles, 2, None, None, None, None, None, None) == bad  # null bindings
    assert "null binding" in _lib.last_error(None)


def test_the_cpp_mirror_declares_the_binding_group():
    import subprocess
    subprocess.run(["g++", "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-fsyntax-only",
                    os.path.join(ROOT, "tests", "cxx", "TestHipBindingGroup.cpp")], check=True)


# ---- the Python layers check before they touch a library ----------------------------------------------------------------------
class _FakeBinding(P.BindingEnergy):
    """A binding with a handle that must never reach the library."""

    def __init__(self, n):
        self._h = 12345
        self.numParticles = n

    def release(self):
        self._h = None


def test_the_group_wrappers_check_their_lists_first(no_library):  # noqa: F811
    bs = [_FakeBinding(4), _FakeBinding(5)]
    many = [_FakeBinding(4) for _ in range(17)]
    pos, frc = [np.zeros((4, 3)), np.zeros((5, 3))], [np.zeros((4, 3)), np.zeros((5, 3))]
    E = P.OpenMMException
    for count, group in ((0, []), (17, many)):
        with pytest.raises(E, match="1 to 16"):
            P.binding_execute_group(group, [1] * count, 99, [2] * count)
        with pytest.raises(E, match="1 to 16"):
            P.binding_energy_group(group, [1] * count, 99, [2] * count)
        with pytest.raises(E, match="1 to 16"):
            P.binding_execute_group_host(group, [np.zeros((4, 3))] * count, [0.5] * count, [np.zeros((4, 3)) for _ in range(count)])
        with pytest.raises(E, match="1 to 16"):
            P.binding_energy_group_host(group, [np.zeros((4, 3))] * count, [0.5] * count)
    twice = [bs[0], bs[0]]
    with pytest.raises(E, match="twice"):
        P.binding_execute_group(twice, [1, 2], 99, [3, 4])
    with pytest.raises(E, match="twice"):
        P.binding_energy_group(twice, [1, 2], 99, [3, 4])
    with pytest.raises(E, match="twice"):
        P.binding_execute_group_host(twice, [pos[0], pos[0]], [0.0, 1.0], [frc[0], frc[0].copy()])
    with pytest.raises(E, match="twice"):
        P.binding_energy_group_host(twice, [pos[0], pos[0]], [0.0, 1.0])
    # mismatched list lengths
    with pytest.raises(E, match="entries"):
        P.binding_execute_group(bs, [1, 2], 99, [3])
    with pytest.raises(E, match="entries"):
        P.binding_execute_group(bs, [1], 99, [3, 4])
    with pytest.raises(E, match="entries"):
        P.binding_execute_group(bs, [1, 2], 99, [3, 4], [5], None)
    with pytest.raises(E, match="entries"):
        P.binding_energy_group(bs, [1, 2], 99, [5, 6], [7])
    with pytest.raises(E):
        P.binding_execute_group_host(bs, pos[:1], [0.0, 1.0], frc)
    with pytest.raises(E):
        P.binding_execute_group_host(bs, pos, [0.0], frc)
    with pytest.raises(E):
        P.binding_energy_group_host(bs, pos, [0.0, 0.5, 1.0])
    with pytest.raises(E):
        P.binding_execute_group_host(bs, pos, [0.0, 1.0], [frc[0], np.zeros((5, 3), dtype=np.float32)])
    with pytest.raises(E):
        P.binding_execute_group_host(bs, [pos[1], pos[1]], [0.0, 1.0], frc)  # wrong number of positions
    # a lambda that is not finite, and a device lambda pointer that is missing
    for bad in (float("nan"), float("inf")):
        with pytest.raises(E, match="finite"):
            P.binding_execute_group_host(bs, pos, [0.0, bad], frc)
        with pytest.raises(E, match="finite"):
            P.binding_energy_group_host(bs, pos, [bad, 1.0])
    with pytest.raises(E):
        P.binding_execute_group(bs, [1, 2], None, [3, 4])
    with pytest.raises(E):
        P.binding_execute_group([bs[0], "not a binding"], [1, 2], 99, [3, 4])
    released = _FakeBinding(4)
    released.release()
    with pytest.raises(E):
        P.binding_execute_group([released], [1], 99, [2])
    # and a valid argument list does go on to the library (the fixture's refusal)
    with pytest.raises(AssertionError, match="reached the library"):
        P.binding_execute_group(bs, [1, 2], 99, [3, 4], [5, None], None)
    with pytest.raises(AssertionError, match="reached the library"):
        P.binding_energy_group_host(bs, pos, [0.0, 1.0])


def test_the_driver_checks_its_arguments_first(no_library):  # noqa: F811
    s = _System()
    bs = [_FakeBinding(4), _FakeBinding(4), _FakeBinding(4)]
    B = md.BindingReplicaMD
    for ladder in ([0.0, 0.5, 0.5], [0.0, 1.0, 0.5], [1.0, 0.5, 0.0], [0.0, float("nan"), 1.0], [0.0, 0.5, float("inf")], [0.0, 1.0],
                   [0.0, "x", 1.0], None):
        with pytest.raises((ValueError, TypeError)):
            B(s, bs, ladder)
    with pytest.raises(ValueError, match="1 to 16"):
        B(s, [_FakeBinding(4) for _ in range(17)], np.linspace(0.0, 1.0, 17))
    with pytest.raises(ValueError, match="1 to 16"):
        B(s, [], [])
    with pytest.raises(ValueError):
        B(s, [_FakeBinding(4), _FakeBinding(5)], [0.0, 1.0])  # bindings of different sizes
    with pytest.raises(ValueError):
        B(s, [_FakeBinding(5), _FakeBinding(5)], [0.0, 1.0])  # (not the system's)
    with pytest.raises(ValueError):
        B(s, [bs[0], bs[1], bs[0]], [0.0, 0.5, 1.0])  # the same binding twice
    with pytest.raises(ValueError):
        B(s, [bs[0], "not a binding", bs[2]], [0.0, 0.5, 1.0])
    with pytest.raises(ValueError):
        B(s, bs, [0.0, 0.5, 1.0], temperatures=[300.0, 300.0])
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            B(s, bs, [0.0, 0.5, 1.0], temperatures=bad)
    # one temperature for all, or one per replica: both go on to the library (the fixture's refusal)
    with pytest.raises(AssertionError, match="reached the library"):
        B(s, bs, [0.0, 0.5, 1.0])
    with pytest.raises(AssertionError, match="reached the library"):
        B(s, bs, [0.0, 0.5, 1.0], temperatures=[300.0, 310.0, 320.0])
