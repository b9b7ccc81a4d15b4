"""MI355X (gfx950) AGBNP / GaussVol implicit-solvent force path behind the reference's AGBNPForce API.

Product code only: HIP kernels + C ABI (csrc/, include/agbnp_hip.h) and the host-side mirror of the
reference's plugin interface (AGBNPplugin.py).  Nothing in this package imports the CPU oracle."""
from .AGBNPplugin import DECOMPOSITION_TERMS, AGBNPContext, AGBNPForce, BindingEnergy, HipCalcAGBNPForceKernel, OpenMMException, energy_group, energy_group_host, execute_group, execute_group_host, host_tables  # noqa: F401
from .AGBNPplugin import decompose_group, decompose_group_host, pair_matrix_group, pair_matrix_group_host  # noqa: F401
from .AGBNPplugin import perturbed_energies_group, perturbed_energies_group_host  # noqa: F401
from .AGBNPplugin import binding_energy_group, binding_energy_group_host, binding_execute_group, binding_execute_group_host  # noqa: F401
from .systems import AGBNPSystem, lattice, load_dms, load_sets, load_system  # noqa: F401
