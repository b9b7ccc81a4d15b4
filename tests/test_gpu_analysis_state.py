"""GPU box: every analysis call path leaves a fast+single context as it found it.  The per-atom planes and the
set-pair matrix are FP64 terms, so a fast+single context runs them with its single-precision option lifted for the call -- by one
guard, on the single-context path (decompose, pair_matrix; device and host) and on the group path (decompose_group, _host).  After
each of the six calls the context's mode, generation and launch counts are what they were, the call is logged as its kind, and
its planes or matrix sum to its energy; at the end the context's own energy is the one it gave before."""
import os

import numpy as np
import pytest

import openmm_agbnp_plugin_amd as P
from openmm_agbnp_plugin_amd import _lib
from tests.gpu_helpers import TIGHT
from tests.gpu_helpers import energy_close as _energy_close
from tests.gpu_helpers import five  # noqa: F401

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _kernel(s, mode="reference", cutoff=None):
    k = P.HipCalcAGBNPForceKernel(device=0, mode=mode)
    force = P.AGBNPForce.from_arrays(*s.params(), version=1)
    if cutoff is not None:
        force.setNonbondedMethod(P.AGBNPForce.CutoffNonPeriodic)
        force.setCutoffDistance(cutoff)
    k.initialize(force)
    return k


def test_every_analysis_path_leaves_a_fast_single_context_as_it_found_it(gpu_required, systems, five):
    torch = pytest.importorskip("torch")
    lib = _lib.load()
    s = systems("trpcage")
    sets, labels = P.load_sets(os.path.join(GOLDEN, "residues_trpcage.txt"))
    S = len(labels)
    k, ref = _kernel(s, "fast+single", 1.0), _kernel(s)
    k.set_atom_sets(sets)
    before = k.energy(s.pos)
    ref.energy(s.pos)

    def state():
        return (lib.agbnp_hip_get_mode(k._h), k.generation(), int(k.scalar("launches")), int(k.scalar("energy_only_launches")))

    recorded = state()
    assert recorded[0] == P.HipCalcAGBNPForceKernel.MODES["fast+single"]

    def after(kind, total, energy):
        print(f"kind {kind}: energy {energy:.9f}, sum {total:.9f}, state {state()}")
        assert state() == recorded
        assert int(k.scalar("last_evaluation_kind")) == kind
        _energy_close(total, energy, TIGHT)

    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    pos = torch.tensor(s.pos, dtype=torch.float64, device=dev).contiguous()
    planes = torch.zeros((2, 4, s.n), dtype=torch.float64, device=dev)
    matrix = torch.zeros((S, S), dtype=torch.float64, device=dev)
    ene = torch.zeros((2,), dtype=torch.float64, device=dev)

    # 1. decompose_device
    k.decompose_device(pos.data_ptr(), planes[1].data_ptr(), ene[1:2].data_ptr(), stream)
    assert k.finish(stream) == 0, (k.withheld(), int(k.scalar("overflow_kinds")))
    after(3, planes[1].sum().item(), ene[1].item())
    # 2. decompose (host)
    e, terms = k.decompose(s.pos)
    after(3, float(terms.sum()), e)
    # 3. pair_matrix_device
    ene.zero_()
    k.pair_matrix_device(pos.data_ptr(), matrix.data_ptr(), ene[1:2].data_ptr(), stream)
    assert k.finish(stream) == 0, (k.withheld(), int(k.scalar("overflow_kinds")))
    after(4, matrix.sum().item(), ene[1].item())
    # 4. pair_matrix (host)
    e, m = k.pair_matrix(s.pos)
    after(4, float(m.sum()), e)
    # 5. decompose_group over [Reference, fast+single]: the Reference member is a launch set of one, the fast+single member runs alone
    planes.zero_()
    ene.zero_()
    P.decompose_group([ref, k], [pos.data_ptr()] * 2, [planes[0].data_ptr(), planes[1].data_ptr()],
                      [ene[0:1].data_ptr(), ene[1:2].data_ptr()], stream)
    assert [ref.finish(stream), k.finish(stream)] == [0, 0]
    assert int(k.scalar("group_members")) == 0
    after(3, planes[1].sum().item(), ene[1].item())
    _energy_close(planes[0].sum().item(), ene[0].item(), TIGHT)
    # 6. decompose_group_host over the same two
    energies, terms = P.decompose_group_host([ref, k], [s.pos, s.pos])
    assert int(k.scalar("group_members")) == 0
    after(3, float(terms[1].sum()), energies[1])
    _energy_close(float(terms[0].sum()), energies[0], TIGHT)

    assert abs(k.energy(s.pos) - before) < 1e-6  # (as test_fast_single_terms_are_those_of_the_fp64_fast_mode compares)
    assert np.isfinite(before)
