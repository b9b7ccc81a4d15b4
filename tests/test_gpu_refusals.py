"""GPU (-m gpu): a refusal of the library surfaces through the Python mirror's call path with the library's own message, read for
the right handle, and leaves the context usable.  The three refusals are host-side argument checks of the engine: nothing is
launched.  fixture264, the smallest bundled system."""
import os

import numpy as np
import pytest

import openmm_agbnp_plugin_amd as P
from openmm_agbnp_plugin_amd import _lib
from tests.gpu_helpers import TIGHT, kernel_of

GOLDEN = np.load(os.path.join(os.path.dirname(__file__), "golden", "golden_vectors.npz"))


@pytest.mark.gpu
def test_a_refused_call_raises_the_librarys_message_and_the_context_goes_on(gpu_required, systems):
    import torch
    s = systems("fixture264")
    k, k2 = kernel_of(s.params()), kernel_of(s.params())
    dev = torch.device("cuda:0")
    p, f, f2 = (torch.zeros((s.n, 3), dtype=torch.float64, device=dev).data_ptr() for _ in range(3))
    e, e2 = (torch.zeros(1, dtype=torch.float64, device=dev).data_ptr() for _ in range(2))
    with pytest.raises(P.OpenMMException, match="agbnp_hip_execute_device: null pointer"):
        k.execute_device(0, 0, 0)
    with pytest.raises(P.OpenMMException, match="agbnp_hip_execute_group: null pointer"):
        P.execute_group([k, k2], [p, 0], [f, f2], [e, e2])
    assert "agbnp_hip_execute_group" in _lib.last_error(k._h)  # kept for the first member ...
    assert "agbnp_hip_execute_group" not in _lib.last_error(k2._h)  # ... and for no other
    binding = P.BindingEnergy(P.AGBNPForce.from_arrays(*s.params(), version=1), range(16))
    with pytest.raises(P.OpenMMException, match="agbnp_hip_binding_execute_device: null pointer"):
        binding.execute_device(0, 0.5, 0)
    assert "agbnp_hip_binding_execute_device" in _lib.last_error(None)  # a binding's messages are those of no context
    # nothing was launched, nothing is pending, and an ordinary evaluation is the committed one
    assert k.finish() == 0 and k2.finish() == 0 and binding.finish() == 0
    forces = np.zeros((s.n, 3))
    energy = k.execute(s.pos, forces)
    assert abs(energy - float(GOLDEN["fixture264_v1_energy"])) < TIGHT
    assert np.abs(forces - GOLDEN["fixture264_v1_forces"]).max() < TIGHT
