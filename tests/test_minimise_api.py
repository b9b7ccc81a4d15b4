"""minimise() of the MD drivers without a device: the argument struct of the FIRE kernels is laid out as the header comment of
csrc/md_kernels.hip states, and bad arguments are refused before any device call."""
import ctypes as C
import os
import re
import types

import pytest

from openmm_agbnp_plugin_amd import md

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "openmm_agbnp_plugin_amd", "csrc", "md_kernels.hip")


def _struct_text():
    text = open(SOURCE).read()
    return text[text.index("struct AgbnpMdFire {"):text.index("};", text.index("struct AgbnpMdFire {"))]


def test_the_struct_is_laid_out_as_the_source_states():
    """The source states: 176 bytes, every field at a multiple of 8 in the order of declaration, 4 bytes of padding behind
    n_min at 152.  The field names and their order are read from the declaration itself."""
    text = _struct_text()
    head = text.splitlines()[0]
    assert "176 bytes" in head and "multiple of 8" in head and "(at 152)" in head and "md.py::_FireArgs" in head
    names = []
    for line in text.splitlines()[1:]:
        decl = line.split("//")[0].strip().rstrip(";")
        if decl:
            names += [re.sub(r"[*\s]", "", part).split(" ")[-1] for part in re.sub(r"^(unsigned|long long|double|int)\s*\*?", "", decl).split(",")]
    assert names == [name for name, _ in md._FireArgs._fields_]
    assert C.sizeof(md._FireArgs) == 176
    assert [getattr(md._FireArgs, name).offset for name in names] == [8 * i for i in range(len(names) - 2)] + [160, 168]
    assert md._FireArgs.n_min.offset == 152 and md._FireArgs.n_min.size == 4
    pointers = ("w", "dt", "alpha", "npos", "iterations", "converged", "voids", "fmax", "coef", "part", "arrived", "log_e", "log_fmax")
    assert names[:13] == list(pointers) and all(getattr(md._FireArgs, name).size == 8 for name in names if name != "n_min")


def test_the_constants_are_fires():
    assert (md.FIRE_F_INC, md.FIRE_F_DEC, md.FIRE_ALPHA0, md.FIRE_F_ALPHA, md.FIRE_N_MIN) == (1.1, 0.5, 0.1, 0.99, 5)
    assert md.MAX_MOVE_LIMIT == 0.5 * md.JUMP_THRESHOLD == 0.02
    assert md.MINIMISE_RECORD.names == ("iterations", "converged", "fmax", "energy", "voids", "withheld")
    for cls in (md.DeviceMD, md.ReplicaMD, md.HamiltonianReplicaMD):
        defaults = cls.minimise.__defaults__
        assert defaults[:6] == (10.0, 1000, 50, 0.001, 0.005, 0.01), cls.__name__
    assert set(md.FIRE_SYMBOLS) == {"agbnp_md_fire_back", "agbnp_md_fire_front"}
    source = open(SOURCE).read()
    assert all(f"int {name}(" in source for name in md.FIRE_SYMBOLS)


class _NoDevice:
    """Stands for a driver whose every device-side attribute raises: a refusal must come before any of them is touched."""

    def __getattr__(self, name):
        raise AssertionError(f"minimise touched `{name}` before refusing its arguments")


BAD = [
    (dict(max_move=0.021), "0.04 nm"),
    (dict(max_move=0.0), "0.04 nm"),
    (dict(tolerance=0.0), "tolerance"),
    (dict(tolerance=-1.0), "tolerance"),
    (dict(tolerance=float("nan")), "tolerance"),
    (dict(dt0=0.0), "dt0"),
    (dict(dt0=-0.001), "dt0"),
    (dict(dt0=0.006), "dt_max"),
    (dict(dt0=0.001, dt_max=0.0005), "dt_max"),
    (dict(max_iterations=0), "max_iterations"),
    (dict(check_every=0), "check_every"),
]


@pytest.mark.parametrize("cls", [md.DeviceMD, md.ReplicaMD, md.HamiltonianReplicaMD], ids=lambda c: c.__name__)
@pytest.mark.parametrize("kw,word", BAD, ids=[",".join(f"{k}={v}" for k, v in kw.items()) for kw, _ in BAD])
def test_bad_arguments_are_refused_before_any_device_call(cls, kw, word):
    with pytest.raises(ValueError, match=re.escape(word)):
        cls.minimise(_NoDevice(), **kw)


def test_the_core_refuses_them_too():
    core = types.SimpleNamespace()
    for kw, word in BAD:
        with pytest.raises(ValueError, match=re.escape(word)):
            md._Replicas.minimise(core, None, 0, None, None, **kw)


def test_the_largest_move_allowed_is_accepted_by_the_check():
    md._check_minimise(10.0, 1, 1, 0.005, 0.005, 0.02)


def test_the_log_asks_for_a_minimisation_first():
    with pytest.raises(RuntimeError, match="minimise\\(\\) has not been called"):
        md._Replicas.minimisation_log(types.SimpleNamespace(fire=None))
