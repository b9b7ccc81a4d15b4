"""ctypes binding of libagbnp_hip.so (C ABI: include/agbnp_hip.h).  There is no fallback: if the shared
library is missing the import of any compute entry point raises, loudly."""
import ctypes as C
import importlib.util
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("AGBNP_HIP_LIBRARY") or os.path.join(_HERE, "libagbnp_hip.so")  # override: diagnostic builds only

OK, ERR_INVALID_ARGUMENT, ERR_PARAMETERS, ERR_DEVICE, ERR_CAPACITY, ERR_TIMEOUT = 0, 1, 2, 3, 4, 5
MAX_GROUP = 16  # AGBNP_HIP_MAX_GROUP: members of one agbnp_hip_execute_group call
MAX_BINDING_GROUP = 16  # AGBNP_HIP_MAX_BINDING_GROUP: bindings of one agbnp_hip_binding_execute_group call
DECOMPOSITION_TERMS = 4  # AGBNP_HIP_DECOMPOSITION_TERMS: planes of agbnp_hip_decompose_*
MAX_SETS = 2048  # AGBNP_HIP_MAX_SETS: sets of a partition (agbnp_hip_set_atom_sets)
MAX_PARAMETER_SETS = 16  # AGBNP_HIP_MAX_PARAMETER_SETS: parameter sets of agbnp_hip_set_parameter_sets

_i, _d, _vp, _dp, _ip, _s = C.c_int, C.c_double, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_char_p
_vpp, _dpp = C.POINTER(C.c_void_p), C.POINTER(_dp)
_create = [_i, _dp, _dp, _dp, _dp, _ip]  # the particle count and the five parameter arrays

# every symbol include/agbnp_hip.h declares: name -> arguments, or (result, arguments) where the result is not an int.  load()
# applies the table and SYMBOLS is its keys: a symbol cannot be exported without its signature (ctypes' default -- int arguments,
# int result -- truncates a 64-bit handle).
SIGNATURES = {
    "agbnp_hip_create": [_vpp, *_create, _i, _i, _d, _i],
    "agbnp_hip_update_parameters": [_vp, *_create],
    "agbnp_hip_execute_host": [_vp, _dp, _dp, _dp],
    "agbnp_hip_execute_device": [_vp, _vp, _vp, _vp, _vp],
    "agbnp_hip_execute_openmm": [_vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _i, _i, _vp],
    "agbnp_hip_energy_host": [_vp, _dp, _dp],
    "agbnp_hip_energy_device": [_vp, _vp, _vp, _vp],
    "agbnp_hip_energy_openmm": [_vp, _vp, _i, _vp, _vp, _i, _vp, _i, _i, _vp],
    "agbnp_hip_decompose_host": [_vp, _dp, _dp, _dp],
    "agbnp_hip_decompose_device": [_vp, _vp, _vp, _vp, _vp],
    "agbnp_hip_set_atom_sets": [_vp, _i, _ip, _i],
    "agbnp_hip_num_atom_sets": [_vp],
    "agbnp_hip_pair_matrix_host": [_vp, _dp, _dp, _dp],
    "agbnp_hip_pair_matrix_device": [_vp, _vp, _vp, _vp, _vp],
    "agbnp_hip_set_parameter_sets": [_vp, _i, _i, _dp, _dp, _dp],
    "agbnp_hip_num_parameter_sets": [_vp],
    "agbnp_hip_perturbed_energies_host": [_vp, _dp, _dp, _dp],
    "agbnp_hip_perturbed_energies_device": [_vp, _vp, _vp, _vp, _vp],
    "agbnp_hip_perturbed_energies_group": [_vpp, _i, _vpp, _vpp, _vpp, _vp],
    "agbnp_hip_perturbed_energies_group_host": [_vpp, _i, _dpp, _dpp, _dp],
    "agbnp_hip_execute_group": [_vpp, _i, _vpp, _vpp, _vpp, _vp],
    "agbnp_hip_execute_group_host": [_vpp, _i, _dpp, _dpp, _dp],
    "agbnp_hip_energy_group": [_vpp, _i, _vpp, _vpp, _vp],
    "agbnp_hip_energy_group_host": [_vpp, _i, _dpp, _dp],
    "agbnp_hip_decompose_group": [_vpp, _i, _vpp, _vpp, _vpp, _vp],
    "agbnp_hip_decompose_group_host": [_vpp, _i, _dpp, _dpp, _dp],
    "agbnp_hip_pair_matrix_group": [_vpp, _i, _vpp, _vpp, _vpp, _vp],
    "agbnp_hip_pair_matrix_group_host": [_vpp, _i, _dpp, _dpp, _dp],
    "agbnp_hip_expect_jump": [_vp],
    "agbnp_hip_atom_order_changed": [_vp],
    "agbnp_hip_finish": [_vp, _vp, _ip],
    "agbnp_hip_poll": [_vp, _ip, _ip],
    "agbnp_hip_wait_verdict": [_vp, _i, _d, _ip, _ip],
    "agbnp_hip_withheld_evaluations": [_vp, _ip, _i],
    "agbnp_hip_generation": (C.c_uint, [_vp]),
    "agbnp_hip_get_scalar": [_vp, _i, _dp],
    "agbnp_hip_get_vector": [_vp, _i, _dp],
    "agbnp_hip_get_table_sizes": [_vp, _ip, _ip],
    "agbnp_hip_get_tables": [_vp, _dp, _dp, _ip, _ip],
    "agbnp_hip_host_tables": [_i, _dp, _ip, _ip, _ip, _dp, _dp, _i, _ip, _ip],
    "agbnp_hip_num_particles": [_vp],
    "agbnp_hip_version": [_vp],
    "agbnp_hip_last_error": (_s, [_vp]),
    "agbnp_hip_destroy": (None, [_vp]),
    "agbnp_hip_device_count": [],
    "agbnp_hip_build_id": (_s, []),
    "agbnp_hip_set_mode": [_vp, _i],
    "agbnp_hip_get_mode": [_vp],
    "agbnp_hip_set_diagnostics": [_vp, _i],
    "agbnp_hip_set_profiling": [_vp, _i],
    "agbnp_hip_num_kernels": [],
    "agbnp_hip_kernel_name": (_s, [_i]),
    "agbnp_hip_get_kernel_times": [_vp, _dp, C.POINTER(C.c_long)],
    "agbnp_hip_binding_create": [_vpp, *_create, _ip, _i, _i, _i, _d, _i],
    "agbnp_hip_binding_execute_device": [_vp, _vp, _d, _vp, _vp, _vp, _vp],
    "agbnp_hip_binding_energy_device": [_vp, _vp, _d, _vp, _vp, _vp],
    "agbnp_hip_binding_execute_host": [_vp, _dp, _d, _dp, _dp, _dp],
    "agbnp_hip_binding_energy_host": [_vp, _dp, _d, _dp, _dp],
    "agbnp_hip_binding_decompose_device": [_vp, _vp, _vp, _vp, _vp],
    "agbnp_hip_binding_decompose_host": [_vp, _dp, _dp, _dp],
    "agbnp_hip_binding_set_atom_sets": [_vp, _i, _ip, _i],
    "agbnp_hip_binding_num_atom_sets": [_vp],
    "agbnp_hip_binding_pair_matrix_device": [_vp, _vp, _vp, _vp, _vp],
    "agbnp_hip_binding_pair_matrix_host": [_vp, _dp, _dp, _dp],
    "agbnp_hip_binding_finish": [_vp, _vp, _ip],
    "agbnp_hip_binding_withheld_evaluations": [_vp, _ip, _i],
    "agbnp_hip_binding_expect_jump": [_vp],
    "agbnp_hip_binding_update_parameters": [_vp, *_create],
    "agbnp_hip_binding_set_mode": [_vp, _i],
    "agbnp_hip_binding_member": (_vp, [_vp, _i]),
    "agbnp_hip_binding_destroy": (None, [_vp]),
    "agbnp_hip_binding_execute_group": [_vpp, _i, _vpp, _vp, _vpp, _vpp, _vpp, _vp],
    "agbnp_hip_binding_energy_group": [_vpp, _i, _vpp, _vp, _vpp, _vpp, _vp],
    "agbnp_hip_binding_execute_group_host": [_vpp, _i, _dpp, _dp, _dpp, _dp, _dp],
    "agbnp_hip_binding_energy_group_host": [_vpp, _i, _dpp, _dp, _dp, _dp],
}
SYMBOLS = list(SIGNATURES)

_lib = None


def _share_hip_runtime_with_torch():
    """One process must hold ONE HIP runtime.  The PyTorch-ROCm wheel bundles its own libamdhip64.so
    (SONAME libamdhip64.so.7) and asks for it by file name, so if this library pulled in /opt/rocm's copy
    first, a later `import torch` would load a second runtime and find no GPU.  Loading torch's copy first
    (without importing torch) makes both resolve to the same object.  Set AGBNP_HIP_SYSTEM_RUNTIME=1 to
    keep the system runtime (processes that never import torch)."""
    if os.environ.get("AGBNP_HIP_SYSTEM_RUNTIME") == "1" or "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        C.CDLL(cand, mode=C.RTLD_GLOBAL)


def load():
    global _lib
    if _lib is not None:
        return _lib
    _share_hip_runtime_with_torch()
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  openmm_agbnp_plugin_amd has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, signature in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the library does not export it
        fn.restype, fn.argtypes = signature if isinstance(signature, tuple) else (C.c_int, signature)
    _lib = lib
    return lib


def build_id():
    """First 16 hex digits of the SHA-256 of the sources the loaded library was built from (csrc/Makefile)."""
    return load().agbnp_hip_build_id().decode()


def last_error(handle=None):
    msg = load().agbnp_hip_last_error(handle)
    return msg.decode() if msg else ""
