"""ReplicaMD (openmm_agbnp_plugin_amd/md.py) at the boundaries that need no device: the host restatements of the
kernels' random numbers and of the exchange rule, the constructor's checks, the symbols of libagbnp_md.so, and the rule that no
kernel source of the tree names a scalar store."""
import ctypes as C
import glob
import math
import os
import re

import numpy as np
import pytest

import openmm_agbnp_plugin_amd as P
from openmm_agbnp_plugin_amd import _lib, md

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("counter,key,expect", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_reproduces_the_random123_known_answers(counter, key, expect):
    assert md.philox4x32(counter, key) == expect
    assert md.philox4x32(np.array(counter, dtype=np.uint32), np.array(key, dtype=np.uint32)) == expect


def test_uniform53_lies_in_the_half_open_interval():
    assert md.uniform53(0, 0) == 2.0 ** -53  # the smallest: never zero, its logarithm is taken
    assert md.uniform53(0xffffffff, 0xffffffff) == 1.0  # the largest
    rng = np.random.default_rng(0)
    for a, b in rng.integers(0, 2 ** 32, size=(2000, 2)):
        u = md.uniform53(a, b)
        assert 0.0 < u <= 1.0
    # 53 bits: the high word shifted by 21 XOR the top 21 bits of the low word
    assert md.uniform53(1, 0) == (2 ** 21 + 1) * 2.0 ** -53
    assert md.uniform53(0, 1 << 11) == 2 * 2.0 ** -53
    # the exchange's deviate is the first two words of the block with counter (k, a lo, a hi, 2)
    w = md.philox4x32((3, 7, 1, 2), (0x12345678, 0x9))
    assert md.exchange_uniform(3, (1 << 32) + 7, (0x9 << 32) | 0x12345678) == md.uniform53(w[0], w[1])


def test_exchange_delta_is_antisymmetric_and_vanishes_at_equal_temperatures():
    rng = np.random.default_rng(1)
    for _ in range(200):
        ka, kb = rng.uniform(1.0, 5.0, 2)
        ua, ub = rng.uniform(-5e4, 5e4, 2)
        d = md.exchange_delta(ka, kb, ua, ub)
        assert md.exchange_delta(kb, ka, ua, ub) == -d  # temperatures swapped
        assert md.exchange_delta(ka, kb, ub, ua) == -d  # energies swapped
        assert md.exchange_delta(kb, ka, ub, ua) == d   # the same pair named the other way round
        assert md.exchange_delta(ka, ka, ua, ub) == 0.0
    # the colder replica (lo) holding the higher energy is always accepted: log(u) <= 0 < Delta
    assert md.exchange_delta(2.0, 3.0, 10.0, -10.0) > 0.0
    assert math.log(md.uniform53(0xffffffff, 0xffffffff)) == 0.0


class _Fake(P.HipCalcAGBNPForceKernel):
    """A kernel with a handle that must never reach the library."""

    def __init__(self, n):
        super().__init__(device=0)
        self._h = 12345
        self.numParticles = n


class _System:
    n = 4
    pos = np.zeros((4, 3))
    ishydrogen = np.zeros(4, dtype=np.int32)


@pytest.fixture()
def no_library(monkeypatch):
    def refuse():
        raise AssertionError("the constructor reached the library")
    monkeypatch.setattr(_lib, "load", refuse)
    monkeypatch.setattr(md, "_MD_LIB", None)


def test_the_constructor_checks_its_arguments_first(no_library):
    s = _System()
    ks = [_Fake(4), _Fake(4), _Fake(4)]
    with pytest.raises(ValueError):
        md.ReplicaMD(s, ks, [300.0, 320.0])  # lists of mismatching length
    with pytest.raises(ValueError):
        md.ReplicaMD(s, ks, [300.0, 320.0, 340.0], seeds=[1, 2])
    with pytest.raises(ValueError):
        md.ReplicaMD(s, [], [])  # R outside 1 .. 16
    with pytest.raises(ValueError):
        md.ReplicaMD(s, [_Fake(4) for _ in range(17)], [300.0 + r for r in range(17)])
    with pytest.raises(ValueError):
        md.ReplicaMD(s, [_Fake(4), _Fake(5)], [300.0, 320.0])  # differing particle counts
    with pytest.raises(ValueError):
        md.ReplicaMD(s, [_Fake(5), _Fake(5)], [300.0, 320.0])  # (not the system's)
    with pytest.raises(ValueError):
        md.ReplicaMD(s, [ks[0], ks[1], ks[0]], [300.0, 320.0, 340.0])  # the same kernel twice
    with pytest.raises(ValueError):
        md.ReplicaMD(s, ks, [300.0, 0.0, 340.0])  # a non-positive temperature
    with pytest.raises(ValueError):
        md.ReplicaMD(s, ks, [300.0, -1.0, 340.0])
    with pytest.raises(ValueError):
        md.ReplicaMD(s, ks, [300.0, float("nan"), 340.0])
    # and a valid argument list does go on to the library (the fixture's refusal, not a ValueError)
    with pytest.raises(AssertionError, match="reached the library"):
        md.ReplicaMD(s, ks, [300.0, 320.0, 340.0])


def test_the_md_library_exports_the_group_symbols():
    lib = C.CDLL(os.path.join(ROOT, "openmm_agbnp_plugin_amd", "libagbnp_md.so"))
    assert md.GROUP_SYMBOLS == ("agbnp_md_group_pre", "agbnp_md_group_mid", "agbnp_md_group_post", "agbnp_md_group_tethers",
                                "agbnp_md_exchange")
    for name in md.GROUP_SYMBOLS:
        getattr(lib, name)  # AttributeError if the library does not export it
    for name in ("agbnp_md_blocks",):
        getattr(lib, name)  # (the grid of one replica: the drivers size their tether partials by it)


def test_the_argument_structs_have_the_kernels_sizes():
    """AgbnpMdGroup / AgbnpMdExchange / AgbnpMdExchangeRecord of csrc/md_kernels.hip: two ints, then 8-byte members only."""
    assert C.sizeof(md._GroupArgs) == 8 + 19 * 8
    assert C.sizeof(md._ExchangeArgs) == 8 + 11 * 8
    assert md.EXCHANGE_RECORD.itemsize == 72
    text = open(os.path.join(ROOT, "openmm_agbnp_plugin_amd", "csrc", "md_kernels.hip")).read()
    for struct in ("AgbnpMdGroup", "AgbnpMdExchange", "AgbnpMdExchangeRecord"):
        assert f"struct {struct} {{" in text


# (spelled in pieces, so that a search of the whole tree for these mnemonics finds nothing, this file included)
_S = "s" + "_"
FORBIDDEN = re.compile("|".join(_S + w for w in ("store" + "_", "buffer" + "_store", "scratch" + "_store", "atomic" + "_", "buffer" + "_atomic",
                                                 "dcache" + "_wb", "dcache" + "_discard")), re.I)


def test_no_kernel_source_names_a_scalar_store():
    sources = glob.glob(os.path.join(ROOT, "**", "*.hip"), recursive=True)
    assert any(p.endswith("md_kernels.hip") for p in sources)
    for path in sources:
        hit = FORBIDDEN.search(open(path, errors="replace").read())
        assert hit is None, f"{os.path.relpath(path, ROOT)} names {hit.group(0)}"
