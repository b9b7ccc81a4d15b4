/* ============================================================================================
 * agbnp_hip.h -- C ABI of the MI355X (gfx950) AGBNP / GaussVol force engine (libagbnp_hip.so).
 *
 * This is the drop-in boundary for ONE hot path of Gallicchio-Lab/openmm_agbnp_plugin: the work
 * behind  AGBNPPlugin::CalcAGBNPForceKernel  (reference: openmmapi/include/AGBNPKernels.h:19-47)
 * for AGBNPForce version 0 (GaussVol/GVolSA) and version 1 (AGBNP1).  Each entry point names the
 * reference interface it replaces.  Plain pointers and sizes only; no C++/torch/OpenMM types.
 *
 * Units: nm, kJ/mol, kJ/mol/nm, elementary charge -- the units of AGBNPForce::addParticle
 * (reference: openmmapi/include/AGBNPForce.h:66-77).
 *
 * Every function returns AGBNP_HIP_OK (0) or an error code; the message is available from
 * agbnp_hip_last_error().  No exception crosses this boundary.
 * ============================================================================================ */
#ifndef AGBNP_HIP_H_
#define AGBNP_HIP_H_

#ifdef __cplusplus
extern "C" {
#endif

typedef struct agbnp_hip_context agbnp_hip_context;

enum agbnp_hip_status {
  AGBNP_HIP_OK = 0,
  AGBNP_HIP_ERR_INVALID_ARGUMENT = 1, /* bad sizes / null pointers / illegal version                */
  AGBNP_HIP_ERR_PARAMETERS = 2,       /* the reference would throw OpenMMException for these params  */
  AGBNP_HIP_ERR_DEVICE = 3,           /* a HIP runtime call failed or no gfx950 device is available  */
  AGBNP_HIP_ERR_CAPACITY = 4,         /* an overlap subtree exceeded the largest supported capacity  */
  AGBNP_HIP_ERR_TIMEOUT = 5           /* agbnp_hip_wait_verdict: the device has not got that far yet */
};

/* nonbonded methods, values of AGBNPForce::NonbondedMethod (openmmapi/include/AGBNPForce.h:44-59) */
enum agbnp_hip_nonbonded_method { AGBNP_HIP_NoCutoff = 0, AGBNP_HIP_CutoffNonPeriodic = 1, AGBNP_HIP_CutoffPeriodic = 2 };

/* Replaces ReferenceCalcAGBNPForceKernel::initialize(system, force)
 * (platforms/reference/src/ReferenceAGBNPKernels.cpp:58-137): takes the per-particle parameters of
 * AGBNPForce::getParticleParameters (radius, gamma, vdw_alpha, charge, ishydrogen), the version
 * (0 = GVolSA, 1 = AGBNP1; 2 = AGBNP2 is out of scope -> AGBNP_HIP_ERR_INVALID_ARGUMENT), the nonbonded method
 * and cutoff (accepted and stored; like the Reference platform the engine evaluates all pairs --
 * see DESIGN.md), builds the I4 tables and uploads everything to device `device`.
 * Fails with AGBNP_HIP_ERR_PARAMETERS and the reference's message if heavy-atom gammas differ
 * (ReferenceAGBNPKernels.cpp:109-116). */
int agbnp_hip_create(agbnp_hip_context** out, int num_particles, const double* radius, const double* gamma,
                     const double* vdw_alpha, const double* charge, const int* ishydrogen, int version,
                     int nonbonded_method, double cutoff_distance, int device);

/* Replaces ReferenceCalcAGBNPForceKernel::copyParametersToContext (ReferenceAGBNPKernels.cpp:1796-1815):
 * gamma, alpha and charge may change; a changed particle count, radius (squared difference > 1e-6) or
 * heavy->hydrogen flip fails with AGBNP_HIP_ERR_PARAMETERS and the reference's message.
 * Drains this context's own stream and every caller stream it has enqueued on since the last agbnp_hip_finish() -- not the
 * device: other contexts keep running -- and rewrites the device copies in place, at unchanged addresses (a captured HIP
 * graph of this context stays valid). */
int agbnp_hip_update_parameters(agbnp_hip_context* ctx, int num_particles, const double* radius, const double* gamma,
                                const double* vdw_alpha, const double* charge, const int* ishydrogen);

/* Replaces ReferenceCalcAGBNPForceKernel::execute (ReferenceAGBNPKernels.cpp:139-149) with the CPU
 * platform's data conventions: positions[3N] in, forces ACCUMULATED into forces[3N] (+=), energy
 * RETURNED in *energy.  Host buffers; synchronous.  Subtree-capacity overflow is handled inside
 * (the evaluation is repeated with the next larger kernel variant). */
int agbnp_hip_execute_host(agbnp_hip_context* ctx, const double* positions, double* forces, double* energy);

/* Device-resident variant for GPU platforms (the data convention of the reference's OpenCL platform,
 * platforms/opencl/src/OpenCLAGBNPKernels.cpp:541-556: forces and energy are ADDED to device
 * buffers, nothing is returned).  d_positions[3N], d_forces[3N], d_energy[1] are FP64 device
 * pointers on the context's device; `stream` is a hipStream_t (NULL = the context's own stream).
 * Asynchronous: FIVE kernel launches for version 1 (since round 5; six where the five-launch mode does not apply -- see
 * below --, one more on systems whose forests do not fit one round of resident tree workgroups), TWO for version 0 (three), no
 * host synchronisation, no allocation once the context has run on its current capacity variant -- any number of
 * evaluations may be queued, or captured into a HIP graph and replayed, before agbnp_hip_finish().
 *
 * Five-launch mode (FP64 row form of the pair stages for version 1, every LDS-resident capacity variant, both device-resident
 * entry points; AGBNP_HIP_FIVE_LAUNCHES=0 turns it off).  There is no preparation launch: the tree launch reads d_positions itself and finds every heavy atom's level-2
 * neighbours through masks that were laid down with a skin (0.08 nm, AGBNP_HIP_MASK_SKIN) at an earlier evaluation; the
 * device renews the masks by itself when a heavy atom has used up a QUARTER of the skin (that evaluation is still exact).
 * What a caller has to know: an evaluation whose positions differ from those of the evaluation before it by more than HALF
 * the skin (0.04 nm) for some heavy atom -- a jump: a minimiser's long step, a Monte-Carlo move, unrelated geometries one
 * after the other -- may have been built from masks that no longer cover it.  It is then WITHHELD exactly like an
 * evaluation that overflowed (nothing added, logged, scalar 15 reports kind 16), the device has already renewed the masks
 * at its positions, and the repeat is right: agbnp_hip_execute_host() repeats by itself, the other entry points' callers
 * through the protocol they already have.  MD steps are two orders of magnitude below the threshold.  Captured graphs
 * keep the mode: from a context's first stream capture on, the device itself names the set of accumulators an evaluation
 * works on, so a replayed evaluation alternates like eager ones do (agbnp_hip_generation() changes once, at that capture).
 * (Run one eager evaluation before the first capture, as for the capacity variant: a context that has never evaluated lays
 * its first masks down with a launch of its own, and a graph that captured that launch repeats it at every replay.)
 * The mode ends for good, silently, where it cannot hold: the diagnostic self volumes, the 32 768-node store in HBM (capacity
 * variant 4), and a stream capture of a context whose pair stages are not the FP64 row form (version 0, the deterministic mode,
 * AGBNP_HIP_ROWS=0, the fast mode's single-precision rows: those keep the mode in eager launches only).  Scalar 16 says which
 * path runs (5 or 6 launches; version 0: 2 or 3).  Since round 6 agbnp_hip_execute_openmm() runs in the mode too (the tree
 * launch reads the context's posq at the context's slots).
 *
 * Forests that outgrow their store are healed inside the tree launch (round 6): the packing of several subtrees into one
 * LDS store is planned from an earlier evaluation's shapes; a forest that does not fit any more used to void the evaluation
 * (withheld, see below) -- now its workgroup builds it again in smaller sets, the evaluation is complete, scalar 17 counts
 * the sets.  What can still be withheld: a subtree that needs the next capacity variant, a neighbour row beyond its walk, a
 * jump (above), a reordered OpenMM context.
 *
 * Overflow contract.  The overlap-tree stage works in fixed-capacity LDS stores; an evaluation whose trees
 * outgrow them (or whose forest packing mispredicted) is INCOMPLETE.  Such an evaluation adds NOTHING to
 * d_forces / d_energy -- the outputs are gated on the device -- and is entered in a log on the device that only
 * agbnp_hip_finish() reads and clears.  So after any number of queued evaluations the caller's buffers hold
 * exactly the sum of the complete ones, and finish() says which ones are missing (the analogue of the reference
 * OpenCL platform's PanicButton protocol, OpenCLAGBNPKernels.cpp:3599-3634: forces invalidated, step retried). */
int agbnp_hip_execute_device(agbnp_hip_context* ctx, const double* d_positions, double* d_forces, double* d_energy,
                             void* stream);

/* The same evaluation in the data conventions of an OpenMM GPU ComputeContext -- what the reference's OpenCL platform
 * kernel reads and writes (platforms/opencl/src/OpenCLAGBNPKernels.cpp:541-556, kernels/GVolReduceTree.cl:92-121):
 *   d_posq            real4 {x, y, z, q} per atom in the CONTEXT's atom order, float4 (posq_is_double = 0) or double4
 *   d_posq_correction float4 low-order parts in mixed precision (position = posq + correction), else NULL
 *   d_atom_index      [N] context slot -> particle index of the System/Force (ComputeContext::getAtomIndexArray);
 *                     NULL = identity
 *   d_force_buffer    the context's 64-bit fixed-point force buffer (value * 2^32), three planes of
 *                     padded_num_atoms words [x | y | z] in context order; forces are ADDED with integer atomics
 *   d_energy_buffer   the context's energy accumulator, double (energy_is_double) or float; the energy is ADDED to
 *                     element energy_slot; NULL = no energy output
 * The same launches as agbnp_hip_execute_device: the engine's first kernel reads posq itself and its last writes the
 * context's buffers.  For that the engine keeps maps of the context's atom order (particle -> slot), built by one small launch
 * when a d_atom_index array is first seen.  OpenMM reorders its atoms now and then (same array, new contents): the first
 * kernel checks the maps against d_atom_index in every evaluation, so the first evaluation after a reorder is WITHHELD
 * like one that overflowed -- nothing of it reaches the context's buffers, agbnp_hip_finish() / agbnp_hip_wait_verdict()
 * report it -- the maps are rebuilt in the next call, and the repeat is right.  Same asynchronous contract, same
 * agbnp_hip_finish(). */
int agbnp_hip_execute_openmm(agbnp_hip_context* ctx, const void* d_posq, int posq_is_double, const void* d_posq_correction,
                             const int* d_atom_index, int padded_num_atoms, long long* d_force_buffer, void* d_energy_buffer,
                             int energy_is_double, int energy_slot, void* stream);

/* Energy-only evaluations: what OpenMM asks of CalcAGBNPForceKernel::execute(context, includeForces = false,
 * includeEnergy = true) -- getState(getEnergy=True) without forces, reporters, Monte-Carlo tests, line searches, the energy
 * matrices of replica exchange.  The three mirror the three execute entry points above, without force outputs:
 *   - NOTHING is written to any force buffer of the caller;
 *   - the energy is the one the matching execute call would produce at the same positions (agbnp_hip_energy_host returns it,
 *     the other two ADD it to *d_energy / to element energy_slot of d_energy_buffer, which must not be NULL);
 *   - such an evaluation is counted in the same overflow log, withheld when incomplete (a subtree that needs the next capacity
 *     variant, a jump of more than 0.04 nm, a reordered OpenMM context), and reported by agbnp_hip_finish(),
 *     agbnp_hip_withheld_evaluations(), agbnp_hip_poll() and agbnp_hip_wait_verdict() under its enqueue index;
 *     agbnp_hip_energy_host() repeats withheld ones itself;
 *   - afterwards the context is in exactly the state a full evaluation leaves (forest packing, neighbour masks and rows, the
 *     healing counters), so full and energy-only evaluations may be interleaved in any order.
 * Five-launch mode with the Reference semantics and the FP64 row form (the default): FOUR launches for version 1 (the cavity
 * launch; the Born rows; the GB stage's energy-only instantiation, which drops the direct force and the Y sums; one small
 * launch with the energy and dealing roles -- no chain-rule and no pseudo-volume launch), TWO for version 0 (the cavity launch;
 * the output launch's role workgroups and mask tiles).  Every other configuration (deterministic, fast and fast+single modes,
 * AGBNP_HIP_ROWS=0, AGBNP_HIP_FIVE_LAUNCHES=0, capacity variant 4, diagnostics, a context that has been stream-captured)
 * runs the full evaluation with its forces sent to a buffer of the context's own: correct, not faster.  Scalar 18 says which.
 * Inside a stream capture these return AGBNP_HIP_ERR_INVALID_ARGUMENT, launch nothing and leave the capture usable:
 * energy-only evaluations are not captured into graphs. */
int agbnp_hip_energy_host(agbnp_hip_context* ctx, const double* positions, double* energy); /* energy RETURNED; synchronous */
int agbnp_hip_energy_device(agbnp_hip_context* ctx, const double* d_positions, double* d_energy, void* stream); /* ADDED; async */
int agbnp_hip_energy_openmm(agbnp_hip_context* ctx, const void* d_posq, int posq_is_double, const void* d_posq_correction,
                            const int* d_atom_index, int padded_num_atoms, void* d_energy_buffer, int energy_is_double,
                            int energy_slot, void* stream); /* ADDED to d_energy_buffer[energy_slot]; async */

/* Per-atom decomposition of an evaluation: which atoms pay the desolvation penalty, per-atom surface areas, per-residue
 * MM-GBSA-style tables.  The energy of an evaluation is an exact sum of four per-atom terms; with nu_i = gamma_i / roffset
 * (roffset: the enlarged-radius increment, float 0.5f * 0.1f promoted; 0 for a hydrogen), B_i the Born radius and
 * k = -(1/2)(1 - 1/80) * 138.935...:
 *   plane 0  "cavity"   nu_i (sv_large_i - sv_vdw_i): the self volumes with the enlarged and the vdW radii.  The plane sums to
 *                       E_vol1 + E_vol2 (scalars 0 + 1); the GaussVol surface area of a heavy atom is A_i = term_i / gamma_i
 *   plane 1  "vdw"      alpha_i / (B_i + 0.14 nm)^3
 *   plane 2  "gb_self"  k q_i^2 / B_i                                        (planes 1 + 2 sum to scalar 2)
 *   plane 3  "gb_pair"  k q_i sum_{j != i} q_j f_ij, f_ij = 1 / sqrt(d^2 + B_i B_j exp(-d^2 / (4 B_i B_j))): each pair shared half
 *                       and half between its atoms.  The plane sums to the GB pair energy (scalar 3)
 * Planes 0..3 summed over all atoms equal the energy the context returns at those positions in its mode.  Version 0 has plane 0
 * only: nothing is added to planes 1..3.  per_atom is term-major: AGBNP_HIP_DECOMPOSITION_TERMS planes of N doubles, atom order.
 *   agbnp_hip_decompose_host    synchronous; per_atom[4 N] is OVERWRITTEN, *energy RETURNED; withheld evaluations are repeated
 *                               inside, as agbnp_hip_energy_host() does
 *   agbnp_hip_decompose_device  asynchronous, no host synchronisation; the 4 N terms are ADDED to d_per_atom and the total to
 *                               *d_energy (d_energy may be NULL): a caller accumulates frames and divides
 * Nothing is written to any force buffer of the caller.  The call counts as ONE evaluation in the context's overflow log under
 * its enqueue index; a withheld one (a jump of more than 0.04 nm, a subtree that needs the next capacity variant, a neighbour row
 * beyond its walk) adds nothing to either output -- gated on the device like every other output -- and agbnp_hip_finish(),
 * _poll(), _wait_verdict() and _withheld_evaluations() report it as they report any other; agbnp_hip_expect_jump() applies.
 * Afterwards the context is in exactly the state a full evaluation leaves: the five-launch mode goes on, scalars 16 and 18 and
 * agbnp_hip_generation() do not change, no later evaluation is withheld for it, and full, energy-only, group and decomposition
 * calls may be interleaved in any order (agbnp_hip_set_diagnostics() is NOT involved).  Scalar 20 reports 3 for it.
 * Launches: the context's energy-only evaluation (four launches for version 1, two for version 0 where scalar 18 is not 0; the
 * full evaluation with its forces sent to a buffer of the context's own elsewhere) with the cavity launch's instantiation that
 * also collects the enlarged-radius self volumes, then ONE launch of the size of the GB stage: all 64 x 64 blocks of atom pairs
 * for plane 3, one thread per atom for planes 0..2.  Every mode is supported.  In the fast mode plane 3 meets only pairs with
 * d^2 < cutoff^2 and the Born radii are that mode's truncated ones (with NoCutoff: the Reference mode's numbers).  In the
 * fast+single mode the terms are FP64: the call computes what the FP64 fast mode gives, and the terms sum to THAT mode's energy
 * (which the call returns), not to the single-precision one.  The deterministic mode gives bit-identical planes from run to run.
 * Inside a stream capture the device call returns AGBNP_HIP_ERR_INVALID_ARGUMENT, launches nothing and leaves the capture
 * usable.  There is no OpenMM-buffer form: decomposition is analysis, not an MD step.  The group form is
 * agbnp_hip_decompose_group() below, the decomposition of a binding energy agbnp_hip_binding_decompose_*(). */
#define AGBNP_HIP_DECOMPOSITION_TERMS 4
int agbnp_hip_decompose_host(agbnp_hip_context* ctx, const double* positions, double* per_atom /*[4][N]*/, double* energy);
int agbnp_hip_decompose_device(agbnp_hip_context* ctx, const double* d_positions, double* d_per_atom /*[4][N]*/,
                               double* d_energy /*may be NULL*/, void* stream);

/* Set-pair interaction matrices: the residue-by-residue (chain-by-chain, receptor-by-ligand) table of an MM-GBSA-style
 * decomposition, which the per-atom planes cannot give -- plane 3 forgets who the partner of a pair was.  A partition assigns
 * every atom to one of S sets; with T[t][i] the four per-atom terms above, k and f_ij as there, the matrix M[S][S] (row-major,
 * FP64) is
 *   a != b   M[a][b] = k sum_{i in a, j in b} q_i q_j f_ij = M[b][a]: the GB pair energy between the two sets is
 *            M[a][b] + M[b][a], shared half and half as plane 3 shares a pair
 *   a == b   M[a][a] = sum_{i in a} (T[0][i] + T[1][i] + T[2][i]) + k sum_{i != j, both in a} q_i q_j f_ij (ordered pairs: every
 *            unordered pair inside the set counts twice)
 * so that row a sums to sum_{i in a} sum_t T[t][i], the whole matrix to the energy the context returns in its mode, M[0][0] of
 * ONE set is that energy, and with every atom its own set the off-diagonal is the bare pair matrix k q_i q_j f_ij.  Version 0
 * fills the diagonal only (the cavity term).  Fast mode: pairs with d^2 < cutoff^2 and that mode's Born radii, exactly as
 * plane 3; fast+single: the FP64 terms of the FP64 fast mode, as for the decomposition.
 *   agbnp_hip_set_atom_sets      the partition: set_of_atom[N] in atom (particle) order like the planes, values 0 .. num_sets - 1,
 *                                num_sets 1 .. AGBNP_HIP_MAX_SETS; sets may be non-contiguous and may be empty (their rows and
 *                                columns stay 0).  A wrong N, a value out of range or a null pointer returns
 *                                AGBNP_HIP_ERR_INVALID_ARGUMENT and the previous partition is kept.  Replaces any earlier
 *                                partition; waits only for work that may be reading the tables it replaces (the context's
 *                                stream and the streams the caller has enqueued on; nothing before the first partition).  It
 *                                changes nothing an evaluation reads: agbnp_hip_generation(), scalars 16 and 18 and the overflow
 *                                log stay as they are, and agbnp_hip_update_parameters() keeps the partition
 *   agbnp_hip_num_atom_sets      S, or 0 when no partition has been set
 *   agbnp_hip_pair_matrix_host   synchronous; matrix[S S] is OVERWRITTEN, *energy RETURNED; withheld evaluations are repeated
 *   agbnp_hip_pair_matrix_device asynchronous, no host synchronisation; the S S entries are ADDED to d_matrix and the total to
 *                                *d_energy (may be NULL): a caller accumulates frames and divides
 * In every respect listed for agbnp_hip_decompose_host / _device above the matrix calls behave as those do: ONE evaluation in the
 * overflow log, gated on the verdict words on the device (a withheld evaluation adds nothing to the matrix or to the energy; the
 * host form repeats it), agbnp_hip_expect_jump() applies, the context is left as a full evaluation leaves it, the calls
 * interleave freely with every other kind, every mode is supported, fast+single is lifted for the call, and inside a stream
 * capture the device call is refused and the capture stays usable.  Scalar 20 reports 4.  Without a partition both return
 * AGBNP_HIP_ERR_INVALID_ARGUMENT and the message says so.
 * Launches: exactly those of agbnp_hip_decompose_device(), with ONE launch of the same grid (k_pair_matrix) in the place of the
 * plane launch.  No pair goes to memory by itself: a tile sums runs of j atoms of one set in registers, the runs in an LDS
 * accumulator by the sets of its two blocks, and leaves with two atomics per pair of sets it met.  The deterministic
 * mode gives a bit-identical matrix from run to run.
 * Not provided: a group form, a binding form, an OpenMM-buffer form.  (Those of the first two were added later, further down:
 * agbnp_hip_pair_matrix_group() and agbnp_hip_binding_pair_matrix_*(); there is still no OpenMM-buffer form.) */
#define AGBNP_HIP_MAX_SETS 2048
int agbnp_hip_set_atom_sets(agbnp_hip_context* ctx, int num_particles, const int* set_of_atom /*[N], 0..num_sets-1*/, int num_sets);
int agbnp_hip_num_atom_sets(const agbnp_hip_context* ctx); /* 0: none set */
int agbnp_hip_pair_matrix_host(agbnp_hip_context* ctx, const double* positions, double* matrix /*[S][S] OVERWRITTEN*/, double* energy);
int agbnp_hip_pair_matrix_device(agbnp_hip_context* ctx, const double* d_positions, double* d_matrix /*[S][S] ADDED*/,
                                 double* d_energy /*may be NULL*/, void* stream);

/* Perturbation energies: what THIS conformation would cost under THOSE parameters -- the cross energies of Hamiltonian replica
 * exchange over gamma / vdw_alpha / charge ladders, the rows of an MBAR / FEP reweighting matrix, a force-field scan -- for up to
 * AGBNP_HIP_MAX_PARAMETER_SETS parameter sets from ONE evaluation.  agbnp_hip_update_parameters() may change only gamma, vdw_alpha
 * and charge; the overlap trees, both sets of self volumes and the Born radii depend on the geometry and the radii alone, and
 * the energy is an explicit function of the three vectors over them (nu, k, B_i and f_ij as for the decomposition above):
 *   E_m = sum_i nu_i^m (sv_large_i - sv_vdw_i)  +  sum_i alpha_i^m / (B_i + 0.14 nm)^3
 *       + k sum_i (q_i^m)^2 / B_i  +  2k sum_{i<j} q_i^m q_j^m f_ij
 * energies[m] is the energy that a context created with (radius, gamma^m, vdw_alpha^m, charge^m, ishydrogen) of this context --
 * the same version, nonbonded method and cutoff -- would return from agbnp_hip_energy_*() at the same positions IN THIS CONTEXT'S
 * MODE.  A hydrogen's gamma counts as 0, as everywhere else; per-atom gammas inside a set are allowed, as
 * agbnp_hip_update_parameters() allows them.  Version 0 gives the cavity term only.
 *   agbnp_hip_set_parameter_sets         the sets: gamma, vdw_alpha, charge are [M][N] row-major, atom (particle) order, M = num_sets
 *                                        1 .. AGBNP_HIP_MAX_PARAMETER_SETS.  A wrong N, M out of range or a null pointer returns
 *                                        AGBNP_HIP_ERR_INVALID_ARGUMENT and the previous sets are kept.  Replaces any earlier sets;
 *                                        waits only for work that may be reading the tables it replaces (the context's stream and
 *                                        the streams the caller has enqueued on; nothing before the first sets).  The sets are
 *                                        independent of the context's own parameters.  It changes nothing an evaluation reads:
 *                                        agbnp_hip_generation(), scalars 16 and 18 and the overflow log stay as they are, and
 *                                        agbnp_hip_update_parameters() keeps the sets
 *   agbnp_hip_num_parameter_sets         M, or 0 when no sets have been set
 *   agbnp_hip_perturbed_energies_host    synchronous; energies[M] is OVERWRITTEN, *energy -- the context's own, under its own
 *                                        parameters -- RETURNED; withheld evaluations are repeated
 *   agbnp_hip_perturbed_energies_device  asynchronous, no host synchronisation; the M energies are ADDED to d_energies and the
 *                                        context's own to *d_energy (may be NULL)
 * In every respect listed for agbnp_hip_decompose_host / _device above the perturbation calls behave as those do: ONE evaluation in
 * the overflow log, gated on the verdict words on the device (a withheld evaluation adds nothing to the energies or to the energy;
 * the host form repeats it), agbnp_hip_expect_jump() applies, the context is left as a full evaluation leaves it, the calls
 * interleave freely with every other kind, every mode is supported, fast+single is lifted for the call, and inside a stream
 * capture the device call is refused and the capture stays usable.  Scalar 20 reports 5.  Without sets both return
 * AGBNP_HIP_ERR_INVALID_ARGUMENT and the message says so.  Fast mode: pairs with d^2 < cutoff^2 and that mode's Born radii;
 * fast+single: the FP64 fast mode's numbers; the deterministic mode gives bit-identical energies from run to run.
 * Launches: exactly those of agbnp_hip_decompose_device(), with ONE launch of the same grid (k_perturb) in the place of the plane
 * launch.  A pair's f_ij -- the FP64 exponential and reciprocal square root -- is formed once and multiplied by M charge products;
 * M is rounded up to a compiled tier (4, 8, 16) whose surplus sets carry zero charges.  The call runs at the context's own
 * positions: no second context, no jump, no hint.
 * Not provided: forces under the other sets, a binding form, an OpenMM-buffer form. */
#define AGBNP_HIP_MAX_PARAMETER_SETS 16
int agbnp_hip_set_parameter_sets(agbnp_hip_context* ctx, int num_particles, int num_sets, const double* gamma /*[M][N]*/,
                                 const double* vdw_alpha /*[M][N]*/, const double* charge /*[M][N]*/);
int agbnp_hip_num_parameter_sets(const agbnp_hip_context* ctx); /* 0: none set */
int agbnp_hip_perturbed_energies_host(agbnp_hip_context* ctx, const double* positions, double* energies /*[M] OVERWRITTEN*/,
                                      double* energy /*the context's own, RETURNED*/);
int agbnp_hip_perturbed_energies_device(agbnp_hip_context* ctx, const double* d_positions, double* d_energies /*[M] ADDED*/,
                                        double* d_energy /*may be NULL*/, void* stream);

/* Replica groups: ONE call that enqueues an evaluation of each of `count` existing contexts (1 .. AGBNP_HIP_MAX_GROUP), for
 * replica exchange, multiple walkers and binding-energy schemes that run several small systems at once.  d_positions,
 * d_forces, d_energies are HOST arrays of `count` DEVICE pointers, one per member.  For every member i the call does exactly
 * what agbnp_hip_execute_device(ctxs[i], d_positions[i], d_forces[i], d_energies[i], stream) would do: the same numbers,
 * forces and energy ADDED, the evaluation counted in THAT member's overflow log under its own enqueue index -- so
 * agbnp_hip_finish(), _poll(), _wait_verdict(), _withheld_evaluations() and _generation() work per member, a withheld member
 * (a jump of more than 0.04 nm, a subtree that needs the next capacity variant) does not affect the others, and group and
 * single-context calls on the same contexts may be interleaved in any order.
 * Members must be distinct contexts on one device, every pointer non-NULL, and the output buffers of different members must
 * not overlap; otherwise AGBNP_HIP_ERR_INVALID_ARGUMENT, nothing is launched and no member changes.  A NULL `stream` means the
 * first member's own stream: the call orders it behind every member's own stream and every member's own stream behind the
 * group's work, so each member's agbnp_hip_finish(NULL) drains it (no member keeps a reference to another member's stream).
 * A caller stream is noted on every member as agbnp_hip_execute_device notes it.  If the call fails with a device error, the
 * members whose launches were not reached are left as they were; a member whose launches failed must be recreated, as after
 * a failed agbnp_hip_execute_device.  Inside a stream capture the call is refused
 * (AGBNP_HIP_ERR_INVALID_ARGUMENT, the capture stays usable): groups are not captured into graphs.
 * Launches.  A member SHARES when its evaluation is exactly the default launch sequence: the five-launch mode with the
 * host-named set (never captured), the Reference semantics, for version 1 the FP64 row form with the forces leaving with the
 * pseudo-volume launch, capacity variant 0-3, no diagnostics, no profiling, AGBNP_HIP_GROUP_LAUNCHES not 0.  Sharing members
 * are split into launch sets by version, capacity variant and the GB far-strip test; each launch set is FIVE launches for
 * version 1 (cavity, Born rows, GB tiles, chain-rule rows, pseudo volumes) or TWO for version 0 (cavity, outputs), whatever
 * its size.  A member's one-off launches (the masks of a fresh context, the words beside the rows after the other entry point)
 * go in front of them.  Every other member runs its ordinary launches on the same stream: correct, not faster.  Members may
 * be different systems or the same system with different parameters.  Scalar 19 says how the last evaluation ran.
 * Argument blocks.  What the shared launches read of a sharing member lives on the device, in the context's own argument block
 * (one per parity of the five-launch mode's sets), rewritten by one small launch only when it changes: a new capacity variant,
 * grown neighbour rows, the other entry point, ANOTHER POSITION BUFFER.  The force and energy pointers travel with each launch,
 * so output buffers may change in every call at no cost; a caller that passes a different d_positions[i] than in the call two
 * group calls before (the same parity) pays one extra small launch for that member.  Keep one position buffer per member (an
 * MD loop does) and a steady run enqueues the five (two) shared launches and nothing else. */
#define AGBNP_HIP_MAX_GROUP 16
int agbnp_hip_execute_group(agbnp_hip_context* const* ctxs, int count, const double* const* d_positions, double* const* d_forces,
                            double* const* d_energies, void* stream);
/* The synchronous twin for host buffers: positions[i][3 n_i] read, forces[i][3 n_i] ACCUMULATED (+=), energies[i] RETURNED.
 * Withheld members are repeated inside, as agbnp_hip_execute_host() does. */
int agbnp_hip_execute_group_host(agbnp_hip_context* const* ctxs, int count, const double* const* positions, double* const* forces,
                                 double* energies);

/* Energy-only replica groups: the conjunction of agbnp_hip_energy_device() and agbnp_hip_execute_group(), for the energy
 * matrices of replica exchange.  d_positions and d_energies are HOST arrays of `count` DEVICE pointers.  For every member i the
 * call does exactly what agbnp_hip_energy_device(ctxs[i], d_positions[i], d_energies[i], stream) would do: the same energy
 * ADDED to *d_energies[i], nothing written to any force buffer of any caller, the evaluation counted in THAT member's overflow
 * log under its own enqueue index, and the member left in the state a full evaluation leaves (forest packing, neighbour masks
 * and rows, healing counters, set parity) -- so agbnp_hip_finish(), _poll(), _wait_verdict(), _withheld_evaluations() and
 * _generation() work per member, a withheld member does not affect the others, and energy groups, full groups and all
 * single-context calls on the same contexts may be interleaved in any order.
 * Arguments as for agbnp_hip_execute_group(): 1 .. AGBNP_HIP_MAX_GROUP distinct contexts on one device, no NULL pointer, the
 * energy words of different members must not overlap (a contiguous array of `count` doubles, one per member, is fine);
 * otherwise AGBNP_HIP_ERR_INVALID_ARGUMENT, nothing is launched and no member changes.  Position buffers MAY be shared between
 * members (two Hamiltonians at one replica's positions): they are inputs.  A NULL `stream`, a caller stream and a device
 * error half-way are handled as in agbnp_hip_execute_group().  Inside a stream capture the call is refused
 * (AGBNP_HIP_ERR_INVALID_ARGUMENT, the capture stays usable).
 * Launches.  A member SHARES under the conditions of agbnp_hip_execute_group() except the one on the forces (no pseudo-volume
 * launch is made, so a system with more forests than one round of tree workgroups shares here): scalar 18 is not 0, the set is
 * named by the host, the positions are the caller's FP64 array, no profiling, AGBNP_HIP_GROUP_LAUNCHES not 0.  Sharing members
 * are split into launch sets by version, capacity variant and the GB far-strip test; a version-1 set is FOUR launches (cavity,
 * Born rows, the GB tiles' energy-only form, three role workgroups per member), a version-0 set TWO (cavity, the output launch
 * without force workgroups), whatever its size; a set of one makes the member's own energy-only launches.  Every other member
 * runs what agbnp_hip_energy_device() runs for it on the same stream: correct, not faster.  Scalars 19 and 20 say how the last
 * evaluation ran.
 * Argument blocks.  Energy groups and full groups build the same block for a member's parity: a steady run that mixes the two
 * kinds of call on the same members with fixed position buffers rewrites nothing (scalar 21 counts the rewrites). */
int agbnp_hip_energy_group(agbnp_hip_context* const* ctxs, int count, const double* const* d_positions, double* const* d_energies,
                           void* stream); /* ADDED to *d_energies[i]; asynchronous */
/* The synchronous twin for host buffers: positions[i][3 n_i] read, energies[i] RETURNED.  Withheld members are repeated inside,
 * alone, as agbnp_hip_energy_host() does. */
int agbnp_hip_energy_group_host(agbnp_hip_context* const* ctxs, int count, const double* const* positions, double* energies);

/* Decomposition groups: the conjunction of agbnp_hip_decompose_device() and agbnp_hip_execute_group(), for per-atom tables that
 * are averaged over replicas or frames and for the decomposition of a binding energy.  d_positions, d_per_atom and d_energies
 * are HOST arrays of `count` DEVICE pointers; d_energies may be NULL altogether (no member's total is wanted).  For every member i
 * the call does exactly what agbnp_hip_decompose_device(ctxs[i], d_positions[i], d_per_atom[i], d_energies[i], stream) would do:
 * the four planes [4][n_i] ADDED to d_per_atom[i] and the total to *d_energies[i], both gated on THAT member's own verdict, ONE
 * evaluation counted in that member's overflow log under its own enqueue index, the member left in the state an energy-only
 * evaluation leaves, scalar 20 reporting 3 -- so agbnp_hip_finish(), _poll(), _wait_verdict(), _withheld_evaluations() and
 * _expect_jump() work per member, a withheld member adds nothing and does not affect the others, and decomposition groups, energy
 * groups, full groups and all single-context calls on the same contexts may be interleaved in any order.
 * Arguments as for agbnp_hip_energy_group(): 1 .. AGBNP_HIP_MAX_GROUP distinct contexts on one device, no NULL pointer (but
 * d_energies as a whole); the plane spans [4 n_i] and the energy words of different members must not overlap one another (a
 * member's energy word must not lie inside its own planes either); otherwise AGBNP_HIP_ERR_INVALID_ARGUMENT -- overlapping planes
 * with a message of their own --, nothing is launched and no member changes.  Position buffers may be shared.  A NULL `stream`, a
 * caller stream and a device error half-way are handled as in agbnp_hip_execute_group().  Inside a stream capture the call is
 * refused (AGBNP_HIP_ERR_INVALID_ARGUMENT, the capture stays usable).
 * Launches.  A member SHARES under the conditions of agbnp_hip_energy_group().  A launch set runs the energy-only group's four
 * launches (version 0: two), the cavity launch in the instantiation that also collects the enlarged-radius self volumes, and
 * behind them ONE plane launch for all its members: FIVE launches (version 0: THREE), whatever its size, where the members'
 * agbnp_hip_decompose_device() calls make five (three) EACH.  A set of one makes the member's own launches.  Every other member
 * -- fast mode, fast+single with the single-precision option lifted for the call, deterministic mode, profiling, a six-launch
 * context, a context captured into a graph before -- runs what agbnp_hip_decompose_device() runs for it on the same stream:
 * correct, not faster.  Scalar 19 says how the last evaluation ran.
 * Argument blocks.  The plane pointers travel with the plane launch, as the force and energy pointers do with theirs: the three
 * kinds of group build the same block for a member's parity, and a steady run that mixes them rewrites nothing (scalar 21). */
int agbnp_hip_decompose_group(agbnp_hip_context* const* ctxs, int count, const double* const* d_positions,
                              double* const* d_per_atom /*[count] x [4][N_m], ADDED*/,
                              double* const* d_energies /*NULL, or [count] words, ADDED*/, void* stream);
/* The synchronous twin for host buffers: positions[i][3 n_i] read, per_atom[i][4 n_i] OVERWRITTEN, energies[i] RETURNED (no NULL
 * pointer; the members' per_atom arrays must not overlap).  Withheld members are repeated inside, alone, as
 * agbnp_hip_decompose_host() does. */
int agbnp_hip_decompose_group_host(agbnp_hip_context* const* ctxs, int count, const double* const* positions,
                                   double* const* per_atom /*overwritten*/, double* energies /*[count]*/);

/* Pair-matrix groups: the conjunction of agbnp_hip_pair_matrix_device() and agbnp_hip_decompose_group(), for set-pair tables that
 * are averaged over replicas or frames and for the pairwise table of a binding energy.  The contract is that of
 * agbnp_hip_decompose_group() with the matrix in the place of the planes.  d_positions, d_matrices and d_energies are HOST arrays
 * of `count` DEVICE pointers; d_energies may be NULL altogether.  For every member i the call does exactly what
 * agbnp_hip_pair_matrix_device(ctxs[i], d_positions[i], d_matrices[i], d_energies[i], stream) would do: the member's OWN partition
 * (S_m may differ between members), its S_m S_m entries ADDED to d_matrices[i] and the total to *d_energies[i], both gated on THAT
 * member's own verdict, ONE evaluation counted in that member's overflow log, scalar 20 reporting 4 and scalar 19 the launch set's
 * size -- so agbnp_hip_finish(), _poll(), _wait_verdict(), _withheld_evaluations() and _expect_jump() work per member, a withheld
 * member adds nothing and does not affect the others, and the call interleaves freely with every other kind of call.
 * Arguments, all checked on the host before anything is launched or any member changes: those of agbnp_hip_decompose_group(); the
 * matrix spans [S_m S_m] and the energy words must not overlap one another, and a member's energy word must not lie inside its own
 * matrix (overlap has a message of its own); a member without a partition is refused with AGBNP_HIP_ERR_INVALID_ARGUMENT and
 * the message says that no partition has been set.  Position buffers may be shared.  Inside a stream capture the call is refused
 * (AGBNP_HIP_ERR_INVALID_ARGUMENT, the capture stays usable).
 * Launches.  A member SHARES under the conditions of agbnp_hip_energy_group(); nothing is added to them.  A launch set runs the
 * decomposition group's first stages -- the energy-only launches with the cavity launch that also collects the enlarged-radius
 * self volumes -- and behind them ONE matrix launch for all its members (k_group_pair_matrix): FIVE launches (version 0: THREE),
 * whatever its size.  A set of one, and every member that cannot share (fast, fast+single, deterministic, profiling, six-launch,
 * captured before), runs what agbnp_hip_pair_matrix_device() runs for it on the same stream.
 * Argument blocks.  The matrix pointers and the members' partitions travel with the matrix launch alone: all four kinds of group
 * build the same block for a member's parity, and a steady run that mixes them rewrites nothing (scalar 21). */
int agbnp_hip_pair_matrix_group(agbnp_hip_context* const* ctxs, int count, const double* const* d_positions,
                                double* const* d_matrices /*[count] x [S_m][S_m], ADDED*/,
                                double* const* d_energies /*NULL, or [count] words, ADDED*/, void* stream);
/* The synchronous twin for host buffers: positions[i][3 n_i] read, matrices[i][S_i S_i] OVERWRITTEN, energies[i] RETURNED (no NULL
 * pointer; the members' matrices must not overlap).  Withheld members are repeated inside, alone, as agbnp_hip_pair_matrix_host()
 * does. */
int agbnp_hip_pair_matrix_group_host(agbnp_hip_context* const* ctxs, int count, const double* const* positions,
                                     double* const* matrices /*overwritten*/, double* energies /*[count]*/);

/* Perturbation groups: the conjunction of agbnp_hip_perturbed_energies_device() and agbnp_hip_decompose_group(), for the energy
 * matrices of Hamiltonian replica exchange and of MBAR over several replicas or frames at once.  The contract is that of
 * agbnp_hip_decompose_group() with the energies under the member's sets in the place of the planes.  d_positions, d_energies and
 * d_own_energies are HOST arrays of `count` DEVICE pointers; d_own_energies may be NULL altogether.  For every member i the call
 * does exactly what agbnp_hip_perturbed_energies_device(ctxs[i], d_positions[i], d_energies[i], d_own_energies[i], stream) would
 * do: the member's OWN sets (M_i may differ between members), its M_i energies ADDED to d_energies[i] and its own energy to
 * *d_own_energies[i], both gated on THAT member's own verdict, ONE evaluation counted in that member's overflow log, scalar 20
 * reporting 5 and scalar 19 the launch set's size -- so agbnp_hip_finish(), _poll(), _wait_verdict(), _withheld_evaluations() and
 * _expect_jump() work per member, a withheld member adds nothing and does not affect the others, and the call interleaves freely
 * with every other kind of call.
 * Arguments, all checked on the host before anything is launched or any member changes: those of agbnp_hip_decompose_group() --
 * 1 .. AGBNP_HIP_MAX_GROUP distinct contexts on one device --; the spans [M_i] and the own-energy words must not overlap one
 * another (overlap has a message of its own); a member without sets is refused with AGBNP_HIP_ERR_INVALID_ARGUMENT and the message
 * says that no parameter sets have been set.  Position buffers may be shared.  Inside a stream capture the call is refused
 * (AGBNP_HIP_ERR_INVALID_ARGUMENT, the capture stays usable).
 * Launches.  A member SHARES under the conditions of agbnp_hip_energy_group(); nothing is added to them.  A launch set runs the
 * decomposition group's first stages and behind them ONE perturbation launch for all its members (k_group_perturb, in the tier of
 * the member with the most sets): FIVE launches (version 0: THREE), whatever its size.  A set of one, and every member that cannot
 * share, runs what agbnp_hip_perturbed_energies_device() runs for it on the same stream.
 * Argument blocks.  The members' tables and output pointers travel with the perturbation launch alone: all five kinds of group build
 * the same block for a member's parity, and a steady run that mixes them rewrites nothing (scalar 21). */
int agbnp_hip_perturbed_energies_group(agbnp_hip_context* const* ctxs, int count, const double* const* d_positions,
                                       double* const* d_energies /*[count] x [M_i], ADDED*/,
                                       double* const* d_own_energies /*NULL, or [count] words, ADDED*/, void* stream);
/* The synchronous twin for host buffers: positions[i][3 n_i] read, energies[i][M_i] OVERWRITTEN, own_energies[i] RETURNED (no NULL
 * pointer; the members' arrays must not overlap).  Withheld members are repeated inside, alone, as
 * agbnp_hip_perturbed_energies_host() does. */
int agbnp_hip_perturbed_energies_group_host(agbnp_hip_context* const* ctxs, int count, const double* const* positions,
                                            double* const* energies /*overwritten*/, double* own_energies /*[count]*/);

/* A hint: the positions of the NEXT evaluation of this context are unrelated to those of the last one (another replica's
 * conformation in an exchange matrix, a restart, a Monte Carlo move).  In the five-launch mode the neighbour masks carry a skin,
 * and a heavy atom that has moved more than 0.04 nm since they were laid down makes the evaluation a jump: withheld, reported
 * as kind 16 by scalar 15, repeated by the caller.  After this call the next evaluation enqueued through ANY entry point
 * (groups included: a member's one-off launches go in front of the shared ones) lays the masks down at its own positions first,
 * with one small launch in front of it exactly as a fresh context's first evaluation does, and is therefore not withheld for
 * the jump.  The hint is consumed by that evaluation.  It costs that one launch and no host synchronisation, and it does not
 * change agbnp_hip_generation().  Where the context does not run the five-launch mode the masks are laid down at every
 * evaluation anyway: the call returns AGBNP_HIP_OK and does nothing.  If the next evaluation is enqueued inside a stream
 * capture the hint stays pending and nothing of it is captured (a captured mask launch would repeat at every replay).
 * The hint only removes the jump verdict.  The evaluation can still be withheld through the usual protocol for a subtree
 * that needs the next capacity variant, a forest packing that the new geometry outgrows, a neighbour row beyond its walk, or
 * a reordered OpenMM context.  Nothing else needs telling: neighbour rows rebuild on the device by themselves and forests heal
 * by themselves. */
int agbnp_hip_expect_jump(agbnp_hip_context* ctx);

/* Binding-energy evaluations: complex, receptor and ligand in ONE call, for BEDAM / single-decoupling protocols, lambda-hybrid
 * forces and the solvation term of MM-GBSA scores.  A binding is made from the N particles of the complex and a set of ligand
 * atoms (1 <= nL < N distinct indices, in any order in the argument and at any places in the complex).  The rest is the receptor;
 * both sub-systems keep ascending complex order.  With x_R and x_L the complex's positions at those atoms and E_RL, E_R, E_L what
 * a context created from the particles of the complex / the receptor / the ligand returns in the binding's mode and version:
 *     u(x)         = E_RL(x) - E_R(x_R) - E_L(x_L)
 *     E_lambda(x)  = E_R + E_L + lambda u = (1 - lambda)(E_R + E_L) + lambda E_RL          dE_lambda / dlambda = u
 *     F_lambda,i   = lambda F^RL_i + (1 - lambda) F^R_r(i)    (i a receptor atom, r(i) its index in the receptor)
 *                  = lambda F^RL_i + (1 - lambda) F^L_l(i)    (i a ligand atom)
 * lambda = 1 is the complex's own evaluation, lambda = 0 the separated pair; lambda is any finite double (values outside [0, 1]
 * extrapolate; NaN or infinity: AGBNP_HIP_ERR_INVALID_ARGUMENT).
 *   agbnp_hip_binding_create             checks every argument on the host before any device call -- the ligand indices (in range,
 *                                        distinct, 1 <= nL < N), the version (0 or 1), the method, the radii: AGBNP_HIP_ERR_INVALID_ARGUMENT
 *                                        -- and creates the three contexts (the reference's equal-gamma error: AGBNP_HIP_ERR_PARAMETERS)
 *   agbnp_hip_binding_execute_device     F_lambda ADDED to d_forces[3N], E_lambda to *d_energy, u to *d_binding_energy (each of the
 *                                        two may be NULL; they must not be the same word); d_positions[3N] the complex's; asynchronous
 *   agbnp_hip_binding_energy_device      the same without forces: NOTHING is written to any force buffer of the caller (d_energy and
 *                                        d_binding_energy may each be NULL, not both)
 *   agbnp_hip_binding_execute_host       synchronous, host buffers: forces ACCUMULATED (+=), the two scalars RETURNED (either pointer
 *   agbnp_hip_binding_energy_host        may be NULL; energy_host: not both); withheld evaluations are repeated inside, as
 *                                        agbnp_hip_execute_host does.  Device evaluations still unfinished are harvested first and
 *                                        reported by the next agbnp_hip_binding_finish, as agbnp_hip_execute_host carries them
 * All or nothing.  A binding evaluation adds F_lambda, E_lambda and u only if ALL THREE members' evaluations completed.  If any
 * member is withheld, for any reason (a jump of more than 0.04 nm, a subtree that needs the next capacity variant, ...), nothing
 * at all reaches the caller's buffers: a hybrid force that is two thirds present would be wrong.  This is decided on the device,
 * with no host read: the launch that adds the outputs reads the three members' verdict words behind their launches.
 * One log.  The k-th binding evaluation since the last agbnp_hip_binding_finish is the k-th evaluation of each member.
 * agbnp_hip_binding_finish drains `stream` (NULL: the complex's own), calls agbnp_hip_finish on the three members and reports as
 * *must_repeat the number of binding evaluations with at least one withheld member; agbnp_hip_binding_withheld_evaluations gives
 * the union of their indices (ascending; -1: null binding).  AGBNP_HIP_ERR_CAPACITY from any member is passed through.  The
 * caller runs the withheld evaluations again and calls finish again, as for a single context.
 * Members.  agbnp_hip_binding_member (0 the complex, 1 the receptor, 2 the ligand; NULL for anything else) lends a member's
 * context for agbnp_hip_get_scalar, agbnp_hip_get_vector, agbnp_hip_poll and agbnp_hip_wait_verdict.  The binding owns it: do not
 * destroy it.  Evaluating or finishing a member directly between two agbnp_hip_binding_finish calls breaks the correspondence of
 * the indices and is NOT ALLOWED; nothing checks for it.
 * Forwarding.  agbnp_hip_binding_update_parameters takes the arrays of the COMPLEX and forwards each member its subset (rules and
 * errors of agbnp_hip_update_parameters); agbnp_hip_binding_set_mode and agbnp_hip_binding_expect_jump forward to all three.
 * Launches.  A full evaluation is ONE gather launch (one thread per receptor or ligand atom copies three doubles out of
 * d_positions through the index map: the complex reads d_positions itself, receptor and ligand read buffers of the binding's own
 * -- also where the ligand is one contiguous range: one rule for every partition), then ONE agbnp_hip_execute_group over
 * {complex, receptor, ligand} whose forces and energies go to buffers of the binding's own, then ONE combine launch (one thread
 * per atom of the complex, one of them for the scalars) that adds the outputs if the three verdicts allow it and clears the
 * binding's buffers WHATEVER the verdict -- a withheld evaluation leaves nothing behind.  The energy-only form: the gather,
 * agbnp_hip_energy_group, a combine of one small workgroup.  The members share launch sets exactly as the members of any group
 * do (by version, capacity variant and far-strip test); a member that cannot share runs its own launches: correct, not faster.
 * A steady run with one d_positions buffer rewrites no argument block (scalar 21 of every member stands still).  Any number of
 * evaluations may be queued before agbnp_hip_binding_finish: stream order protects the binding's buffers, so use ONE stream
 * between two finish calls.  The combine is elementwise: in the deterministic mode the outputs are bit-identical from run to run.
 * Inside a stream capture the device calls return AGBNP_HIP_ERR_INVALID_ARGUMENT, launch nothing and leave the capture usable:
 * they use group calls, and groups are not captured into graphs.
 * Every failure of a binding call leaves its message with the calling thread: agbnp_hip_last_error with a NULL context.
 * No OpenMM-buffer form; groups of several bindings: below. */
typedef struct agbnp_hip_binding agbnp_hip_binding;
int agbnp_hip_binding_create(agbnp_hip_binding** out, int num_particles, const double* radius, const double* gamma,
                             const double* vdw_alpha, const double* charge, const int* ishydrogen, const int* ligand_atoms,
                             int num_ligand_atoms, int version, int nonbonded_method, double cutoff_distance, int device);
int agbnp_hip_binding_execute_device(agbnp_hip_binding* b, const double* d_positions, double lambda, double* d_forces, double* d_energy,
                                     double* d_binding_energy, void* stream); /* F_lambda, E_lambda, u ADDED; asynchronous */
int agbnp_hip_binding_energy_device(agbnp_hip_binding* b, const double* d_positions, double lambda, double* d_energy,
                                    double* d_binding_energy, void* stream); /* no force written */
int agbnp_hip_binding_execute_host(agbnp_hip_binding* b, const double* positions, double lambda, double* forces, double* energy,
                                   double* binding_energy);
int agbnp_hip_binding_energy_host(agbnp_hip_binding* b, const double* positions, double lambda, double* energy, double* binding_energy);
/* Per-atom decomposition of a binding energy: which receptor and ligand atoms carry u.  With T_RL, T_R, T_L the four planes of
 * agbnp_hip_decompose_*() of the complex, the receptor and the ligand at the complex's positions,
 *   D[t][i] = T_RL[t][i] - T_own[t][own(i)],   t = 0..3, i an atom of the complex,
 * T_own the receptor's plane at i's index in the receptor if i is a receptor atom, else the ligand's at i's index in the ligand.
 * Every member's planes sum to its energy, so sum_{t,i} D[t][i] = u; plane t of D summed is that term's share of u.  There is no
 * lambda.  Version 0 has plane 0 only.  per_atom is term-major: AGBNP_HIP_DECOMPOSITION_TERMS planes of N doubles, the
 * complex's atom order.
 *   agbnp_hip_binding_decompose_device  asynchronous; the 4 N terms are ADDED to d_per_atom and u to *d_binding_energy (may be
 *                                       NULL) -- all of it or, if ANY of the three members' evaluations is withheld, nothing:
 *                                       one verdict, read on the device
 *   agbnp_hip_binding_decompose_host    synchronous; per_atom[4 N] OVERWRITTEN, *binding_energy RETURNED (may be NULL); withheld
 *                                       evaluations are repeated inside, up to ten times, as agbnp_hip_binding_energy_host
 * An evaluation is three steps on one stream: the gather launch of every binding evaluation, ONE agbnp_hip_decompose_group() over
 * {complex, receptor, ligand} -- where the three share a launch set: five launches (version 0: three) -- into a staging buffer of
 * the binding's own (made at the first decomposition call), and one combine launch, which reads the three verdicts, adds D and
 * u, and clears the staging words whatever the verdict: 1 + 5 + 1 launches.  It is ONE binding evaluation of the one log above:
 * the k-th binding evaluation is the k-th evaluation of each member whichever kind it is, agbnp_hip_binding_finish and
 * _withheld_evaluations report it like the others, _expect_jump applies, and it may be interleaved with the other binding
 * calls in any order on one stream.  Every mode works as the members' own decompositions do.  Inside a stream capture the call
 * is refused before anything is launched.  If the members' group call fails, no combine launch is made and the staging buffer
 * is cleared on the stream.  Not provided: a decomposition inside binding groups, an OpenMM-buffer form, residue bookkeeping --
 * the planes are per atom, the caller sums them. */
int agbnp_hip_binding_decompose_device(agbnp_hip_binding* b, const double* d_positions, double* d_per_atom /*[4][N], ADDED*/,
                                       double* d_binding_energy /*may be NULL; u ADDED*/, void* stream);
int agbnp_hip_binding_decompose_host(agbnp_hip_binding* b, const double* positions, double* per_atom /*overwritten*/,
                                     double* binding_energy);
/* Set-pair matrix of a binding energy: which receptor set pays how much against which ligand set, and how much the ligand's
 * arrival changes the interaction of two receptor sets -- the pairwise table of an MM-GBSA decomposition, which the per-atom
 * planes above cannot give.  A partition over the atoms of the COMPLEX (S sets, 1 .. AGBNP_HIP_MAX_SETS; sets may mix receptor
 * and ligand atoms) is restricted to each member through the binding's index maps, with the SAME set numbering and the SAME S:
 * a set with no atom in a member is an empty set there.  With M_RL, M_R, M_L the members' matrices of agbnp_hip_pair_matrix_*()
 * at the complex's positions, each S x S,
 *   D[a][b] = M_RL[a][b] - M_R[a][b] - M_L[a][b],   sum_{a,b} D[a][b] = u = E_RL - E_R - E_L.
 * D is symmetric; row a sums to sum_{i in a} sum_t D[t][i] of agbnp_hip_binding_decompose_*(); for a set a wholly in the receptor
 * and a set b wholly in the ligand D[a][b] = M_RL[a][b], the direct GB interaction; for two receptor sets D[a][b] is what the
 * ligand's presence changes of their interaction.  Version 0 fills the diagonal only.  There is no lambda.
 *   agbnp_hip_binding_set_atom_sets      the partition, set_of_atom[N] in the complex's atom order, validated entirely on the
 *                                        host first: a refused one (wrong N, a value outside 0 .. num_sets - 1, num_sets out of
 *                                        range, a null pointer) leaves the previous partition in force in all three members.
 *                                        agbnp_hip_binding_update_parameters() keeps the partition
 *   agbnp_hip_binding_num_atom_sets      S, or 0 when none has been set
 *   agbnp_hip_binding_pair_matrix_device asynchronous; the S S entries of D are ADDED to d_matrix and u to *d_binding_energy
 *                                        (may be NULL) -- all of it or, if ANY member's evaluation is withheld, nothing
 *   agbnp_hip_binding_pair_matrix_host   synchronous; matrix[S S] OVERWRITTEN, *binding_energy RETURNED (may be NULL); withheld
 *                                        evaluations are repeated inside, up to ten times
 * An evaluation is the three steps of the binding decomposition on one stream: the gather launch, ONE
 * agbnp_hip_pair_matrix_group() over {complex, receptor, ligand} -- where the three share a launch set: five launches (version
 * 0: three) -- into a staging buffer of the binding's own, and one combine launch (one thread per cell), which reads the three
 * verdicts, adds D and u only if all three completed, and clears the staging words whatever the verdict: 1 + 5 + 1 launches.
 * The staging buffer holds [3][S][S] doubles and three energy words: 24 S^2 bytes -- 1.6 MB for 258 residues, 100 MB at 2048
 * sets.  It is made at the first matrix call and remade when S changes, after the streams that may read it have drained.
 * It is ONE binding evaluation of the one log above: agbnp_hip_binding_finish, _withheld_evaluations and _expect_jump apply, and
 * the call may be interleaved with the other binding calls in any order on one stream.  The combine is elementwise: in the
 * deterministic mode D is bit-identical from run to run.  Without a partition both forms return
 * AGBNP_HIP_ERR_INVALID_ARGUMENT and the message says that no partition has been set.  Inside a stream capture the call is
 * refused before anything is launched.  If the members' group call fails, no combine launch is made and the staging buffer is
 * cleared on the stream.  Not provided: a matrix inside binding groups, an OpenMM-buffer form. */
int agbnp_hip_binding_set_atom_sets(agbnp_hip_binding* b, int num_particles, const int* set_of_atom /*[N] complex order*/, int num_sets);
int agbnp_hip_binding_num_atom_sets(const agbnp_hip_binding* b); /* 0: none set */
int agbnp_hip_binding_pair_matrix_device(agbnp_hip_binding* b, const double* d_positions, double* d_matrix /*[S][S], ADDED*/,
                                         double* d_binding_energy /*may be NULL; u ADDED*/, void* stream);
int agbnp_hip_binding_pair_matrix_host(agbnp_hip_binding* b, const double* positions, double* matrix /*overwritten*/,
                                       double* binding_energy /*may be NULL*/);
int agbnp_hip_binding_finish(agbnp_hip_binding* b, void* stream, int* must_repeat);
int agbnp_hip_binding_withheld_evaluations(const agbnp_hip_binding* b, int* indices, int capacity);
int agbnp_hip_binding_expect_jump(agbnp_hip_binding* b);
int agbnp_hip_binding_update_parameters(agbnp_hip_binding* b, int num_particles, const double* radius, const double* gamma,
                                        const double* vdw_alpha, const double* charge, const int* ishydrogen);
int agbnp_hip_binding_set_mode(agbnp_hip_binding* b, int mode);
agbnp_hip_context* agbnp_hip_binding_member(agbnp_hip_binding* b, int which); /* 0 complex, 1 receptor, 2 ligand */
void agbnp_hip_binding_destroy(agbnp_hip_binding* b);

/* Binding groups: ONE call that enqueues an evaluation of each of `count` bindings (1 .. AGBNP_HIP_MAX_BINDING_GROUP), for lambda
 * ladders -- BEDAM and single-decoupling replica exchange over E_lambda = E_R + E_L + lambda u -- and for scoring several
 * complexes at once.  The contract of agbnp_hip_execute_group(), carried over to bindings: for every binding k
 * the call does exactly what agbnp_hip_binding_execute_device(bindings[k], d_positions[k], lambda_k, d_forces[k], d_energies[k],
 * d_binding_energies[k], stream) does (the energy forms: agbnp_hip_binding_energy_device()), with the same numbers.  F_lambda,
 * E_lambda and u are ADDED.  All or nothing holds PER BINDING: a binding with a withheld member adds nothing and leaves nothing
 * behind, the other bindings of the call are not affected.  The evaluation is the next one of each binding's own log:
 * agbnp_hip_binding_finish(), _withheld_evaluations, _expect_jump and _member work per binding, and group calls and single calls
 * on the same bindings may be interleaved in any order.  The bindings need not be the same complex.
 * Arguments.  d_positions, d_forces, d_energies, d_binding_energies are HOST arrays of `count` DEVICE pointers.  Entries of
 * d_energies / d_binding_energies may be NULL, and so may the two arrays (every entry NULL); in the energy form the two entries of
 * one binding may not both be NULL and may not be the same word.  Position buffers MAY be shared between bindings (two rungs
 * scored at one conformation); the outputs of two bindings -- forces [3 N_k], energy words, u words, each against every other --
 * must not overlap.
 * d_lambdas is a DEVICE array of `count` doubles.  The combine launch reads it WHEN IT RUNS, in stream order: a kernel enqueued
 * earlier on the same stream may have written it, with no host call in between (a lambda exchange decided on the device).  The
 * values are not checked on the device.  The host forms take a host array and check every value for finiteness.
 * Errors.  Checked on the host before anything is launched or any binding changes, AGBNP_HIP_ERR_INVALID_ARGUMENT with the message
 * in the thread's agbnp_hip_last_error(NULL): count outside 1 .. 16, a NULL binding, the same binding twice, bindings on different
 * devices, a NULL position or force pointer, overlapping outputs.  Inside a stream capture the call is refused, launches nothing
 * and leaves the capture usable.
 * Launches.  ONE gather launch over the atoms of all bindings, the members' evaluations through agbnp_hip_execute_group() /
 * agbnp_hip_energy_group() -- ONE call over all members where 3 count <= AGBNP_HIP_MAX_GROUP, else THREE, by kind: all complexes,
 * all receptors, all ligands (same-kind members of one system have the same version and, at related geometries, the same capacity
 * variant: one launch set each) --, ONE combine launch over all bindings.  A ladder of 16 rungs: 1 + 3 x 5 + 1 = 17 launches
 * where 16 single calls make 112.  With a NULL stream the work is ordered on the first binding's complex's own stream and every
 * binding's agbnp_hip_binding_finish(b, NULL, ..) drains it.
 * The host forms stage the inputs, run the device path and finish; forces are ACCUMULATED (+=), energies[k] and
 * binding_energies[k] RETURNED (either array may be NULL; the energy form: not both).  A binding whose evaluation was withheld is
 * repeated alone, as agbnp_hip_binding_execute_host() repeats; unfinished device evaluations are carried to the next finish. */
#define AGBNP_HIP_MAX_BINDING_GROUP 16
int agbnp_hip_binding_execute_group(agbnp_hip_binding* const* bindings, int count, const double* const* d_positions,
                                    const double* d_lambdas, double* const* d_forces, double* const* d_energies,
                                    double* const* d_binding_energies, void* stream);
int agbnp_hip_binding_energy_group(agbnp_hip_binding* const* bindings, int count, const double* const* d_positions,
                                   const double* d_lambdas, double* const* d_energies, double* const* d_binding_energies,
                                   void* stream);
int agbnp_hip_binding_execute_group_host(agbnp_hip_binding* const* bindings, int count, const double* const* positions,
                                         const double* lambdas, double* const* forces, double* energies, double* binding_energies);
int agbnp_hip_binding_energy_group_host(agbnp_hip_binding* const* bindings, int count, const double* const* positions,
                                        const double* lambdas, double* energies, double* binding_energies);

/* Tells the engine that the contents of the d_atom_index array it last saw have changed (OpenMM has reordered its atoms):
 * the next agbnp_hip_execute_openmm() rebuilds its maps first, and no evaluation is lost to the check.  Optional -- without
 * it the first evaluation after a reorder is withheld and repeated, see above. */
int agbnp_hip_atom_order_changed(agbnp_hip_context* ctx);

/* Waits for `stream`, then reads and clears the overflow log.  *must_repeat = the number of evaluations enqueued
 * since the previous agbnp_hip_finish() whose outputs were withheld (0: every one is complete and in the caller's
 * buffers).  If it is not 0 the context has already prepared the repeat (one subtree per workgroup, and the next
 * larger capacity variant if a single subtree did not fit): the caller runs those evaluations again -- their
 * positions in enqueue order come from agbnp_hip_withheld_evaluations() -- and calls finish() again.
 * Returns AGBNP_HIP_ERR_CAPACITY if a subtree exceeds the largest variant. */
int agbnp_hip_finish(agbnp_hip_context* ctx, void* stream, int* must_repeat);

/* Which evaluations the LAST agbnp_hip_finish() found withheld: writes up to `capacity` indices (0 = the first
 * evaluation enqueued through a device-resident entry point after the finish before it; the log's bitmap names the first
 * 2048 evaluations since that finish -- fewer by the agbnp_hip_execute_host calls in between, whose evaluations take the first
 * entries -- later ones are only counted)
 * and returns their total number (-1: null context). */
int agbnp_hip_withheld_evaluations(const agbnp_hip_context* ctx, int* indices, int capacity);

/* Non-blocking look at the overflow log (no device call, no synchronisation): how many of the evaluations enqueued since
 * the last agbnp_hip_finish() have COMPLETED on the device and how many of those were withheld, read from pinned host
 * memory that the device writes at the end of every evaluation.  A caller that must not stall its stream every step (an MD
 * loop) polls this after each enqueue and calls agbnp_hip_finish() only when *withheld is non-zero (or now and then: the
 * log names the first 2048 evaluations since the last finish, see agbnp_hip_withheld_evaluations).  What it learns is at least one evaluation old.  The reference's GPU platform does a
 * blocking read every step instead (OpenCLAGBNPKernels.cpp:3599-3634).  AGBNP_HIP_ERR_DEVICE: no pinned memory. */
int agbnp_hip_poll(const agbnp_hip_context* ctx, int* evaluations_completed, int* withheld);

/* The strict per-step check without draining the stream.  Blocks the calling HOST thread (no device call, nothing is
 * synchronised) until the device has delivered its verdict on `evaluations` evaluations since the last agbnp_hip_finish()
 * (0 or less: on every evaluation enqueued through this library's entry points since then; a caller that replays captured
 * graphs passes its own count) or `timeout_seconds` have passed, by watching the pinned status words of agbnp_hip_poll().
 * An evaluation's verdict -- complete, or withheld because a tree outgrew its store -- is final when its tree stage has
 * ended, about three quarters into the evaluation, and is written there; the forces follow on the stream, gated on the
 * device by the same words.  So *withheld == 0 on return means every one of those evaluations WILL add its forces and
 * energy, in stream order, and the caller may go on enqueuing work behind them; *withheld != 0 means what it means
 * after agbnp_hip_finish(): call it, then repeat.  This is the reference GPU platform's protocol (a blocking read of the
 * overflow flag in every step, OpenCLAGBNPKernels.cpp:3599-3634) with the same guarantee and without its pipeline drain:
 * the host waits for a word, not for the stream.  AGBNP_HIP_ERR_TIMEOUT: not there yet (the outputs are valid as far as
 * they go); AGBNP_HIP_ERR_DEVICE: no pinned memory. */
int agbnp_hip_wait_verdict(const agbnp_hip_context* ctx, int evaluations, double timeout_seconds, int* evaluations_completed,
                           int* withheld);

/* Changes whenever kernel arguments that a captured HIP graph of agbnp_hip_execute_device has frozen go stale:
 * after a finish() that raised the capacity variant or grew the scratch pools.  A caller that replays a graph
 * compares the value at capture time with the current one after every finish() and re-captures on a difference.
 * agbnp_hip_update_parameters() does NOT change it: parameters are rewritten in place at unchanged addresses.
 * Mixing entry points invalidates captured graphs (five-launch mode): the tree launch finds a work item's root through words
 * that hold the root's SLOT in the context's order for agbnp_hip_execute_openmm and its atom index for
 * agbnp_hip_execute_device / _host, rewritten for whichever entry point enqueued last.  A graph has frozen the kernel that
 * reads them one way, so the value also changes whenever those words change their kind: an evaluation through the other
 * entry point (eager or captured), a reordered OpenMM context, a withheld evaluation of a context that runs through
 * agbnp_hip_execute_openmm (the repeat's packing is laid down by the host).  Compare it after every call that enqueues through
 * another entry point as well, BEFORE the next replay: nothing on the device catches a stale replay (slots and atom indices
 * are both below N), its forces are simply wrong.  Read the value to keep AFTER the capture has ended. */
unsigned agbnp_hip_generation(const agbnp_hip_context* ctx);

/* Evaluation mode (default 0 = the Reference platform's semantics: the descreening sums reach as far as the tables,
 * 2 nm, GB meets ALL pairs, nonbonded method and cutoff are inert -- parity target of this engine).
 * AGBNP_HIP_MODE_FAST = the semantics of the reference's GPU (OpenCL) platform: every pair stage of AGBNP1 -- Born-radius
 * descreening sums, GB pair energy / direct forces / Y sums, chain-rule W/U sums and forces -- only meets pairs with
 * r^2 < cutoff_distance^2 (platforms/opencl/src/kernels/AGBNPBornRadii.cl:268,430, AGBNPGBEnergy.cl:145,186).  As on
 * that platform the cutoff only exists for a nonbonded method other than NoCutoff (USE_CUTOFF, OpenCLAGBNPKernels.cpp:487,
 * 1149-1150): with NoCutoff the fast mode truncates nothing and computes exactly what the Reference mode does.
 * CutoffPeriodic is rejected (AGBNP_HIP_ERR_INVALID_ARGUMENT): no periodic box crosses this boundary.  Tiles beyond the
 * cutoff are culled.
 * FP64 throughout; version 0 has no pair stage and is unaffected.  For comparisons with the OpenCL plugin; results
 * differ from the Reference platform by the truncated pairs.  Drains this context's own stream (not the device); bumps
 * agbnp_hip_generation().
 *
 * AGBNP_HIP_MODE_DETERMINISTIC (may be combined with either): bit-identical results from run to run.  By default sums
 * that many workgroups contribute to are FP64 atomics whose order is not fixed, so results differ by ~1e-16 relative
 * between runs.  In this mode every term that enters an order-dependent sum is first rounded to a fixed quantum
 * (2^-34 kJ/mol/nm for forces, 2^-52 nm^3 for self volumes, 2^-44 / 2^-40 for the pair-stage sums, 2^-36 kJ/mol for
 * energies): sums of such terms are exact in FP64, hence independent of their order.  Results stay within 1e-8 of the
 * default mode's (far inside the 1e-4 parity bar).
 *
 * AGBNP_HIP_MODE_SINGLE (only together with AGBNP_HIP_MODE_FAST): the pair stages compute their pair terms in single
 * precision (hardware exp2 / rsqrt; positions relative to a local origin before they are rounded), as the reference's
 * OpenCL platform does in its default precision (AGBNPBornRadii.cl:181-430, AGBNPGBEnergy.cl are all-float).  In the row
 * form -- where the fast mode normally runs -- that is all three of them: descreening sums, GB, chain rule (the spline table
 * as FP32 in LDS); in the tile form (no neighbour lists: NoCutoff, AGBNP_HIP_ROWS=0) the GB strips only.  The sums of a
 * slice or tile run in FP32, everything that leaves a wave, the Born-radius algebra, the trees and the energies stay
 * FP64.  Forces differ from the FP64 fast mode by ~5e-4 kJ/mol/nm, the energy by ~3e-3 kJ/mol on a 4000-atom protein.
 * Rejected without AGBNP_HIP_MODE_FAST: the Reference semantics are FP64. */
enum agbnp_hip_mode { AGBNP_HIP_MODE_REFERENCE = 0, AGBNP_HIP_MODE_FAST = 1, AGBNP_HIP_MODE_DETERMINISTIC = 2, AGBNP_HIP_MODE_SINGLE = 4 };
int agbnp_hip_set_mode(agbnp_hip_context* ctx, int mode);
int agbnp_hip_get_mode(const agbnp_hip_context* ctx);

/* Diagnostics of the LAST completed evaluation (test support; mirrors the quantities the reference
 * prints at verbose_level > 0, ReferenceAGBNPKernels.cpp:333-352,459-462,519).  `which` of agbnp_hip_get_scalar is one of
 * enum agbnp_hip_scalar, `which` of agbnp_hip_get_vector one of enum agbnp_hip_vector. */
enum agbnp_hip_scalar {
  AGBNP_HIP_SCALAR_E_VOL1 = 0,
  AGBNP_HIP_SCALAR_E_VOL2 = 1,
  AGBNP_HIP_SCALAR_E_ATOM = 2,             /* vdW + GB self */
  AGBNP_HIP_SCALAR_E_GB_PAIR = 3,
  AGBNP_HIP_SCALAR_MAX_SUBTREE_NODES = 4,
  AGBNP_HIP_SCALAR_TOTAL_NODES = 5,        /* total tree nodes */
  AGBNP_HIP_SCALAR_VARIANT = 6,            /* kernel variant */
  AGBNP_HIP_SCALAR_MAX_LOCAL_ATOMS = 7,
  AGBNP_HIP_SCALAR_FORESTS = 8,            /* work slots (forests) planned for the next evaluation */
  AGBNP_HIP_SCALAR_ROWS_ON = 9,            /* 1 if the range-limited pair stages run in row form (neighbour rows with a skin, rebuilt on
                                            * the device when an atom has moved more than half the skin; Reference mode, version 1) */
  AGBNP_HIP_SCALAR_ROW_BUILDS = 10,        /* builds of those rows so far */
  AGBNP_HIP_SCALAR_PACK_LEVEL = 11,        /* forest packing: how far the assumed store capacity is tightened (0 = not at all; one step of
                                            * 15 % when healed forests keep coming or one could not be healed, given back after clean
                                            * plans in a row -- more of them every time) */
  AGBNP_HIP_SCALAR_PACK_AGE = 12,          /* evaluations since the packing was planned */
  AGBNP_HIP_SCALAR_ROW_SLICE = 13,         /* entries per slice of a neighbour row (one wave of a row launch walks one slice; tuned on
                                            * the device) */
  AGBNP_HIP_SCALAR_PACK_PLANS = 14,        /* forest packings planned so far (a packing in use is planned anew every
                                            * AGBNP_HIP_REPLAN_EVERY-th evaluation, default 16, or when the trees have drifted from the
                                            * shapes it was planned for) */
  AGBNP_HIP_SCALAR_OVERFLOW_KINDS = 15,    /* why the last agbnp_hip_finish() withheld evaluations: bits of enum agbnp_hip_overflow_kind */
  AGBNP_HIP_SCALAR_LAUNCHES = 16,          /* kernel launches of an evaluation as the context runs now: version 1: 5 (five-launch mode)
                                            * or 6; version 0: 2 or 3 */
  AGBNP_HIP_SCALAR_HEALED_FORESTS = 17,    /* forests that outgrew their store and were healed inside the tree launch (built again in
                                            * smaller sets: the evaluation is complete, nothing is withheld for them) over the
                                            * evaluations the last agbnp_hip_finish() covered */
  AGBNP_HIP_SCALAR_ENERGY_ONLY_LAUNCHES = 18,  /* kernel launches of an energy-only evaluation as the context runs now: 4 (version 1) or
                                            * 2 (version 0), 0 where it runs as a full evaluation with its forces sent to a buffer of
                                            * the context's own */
  AGBNP_HIP_SCALAR_GROUP_MEMBERS = 19,     /* members of the launch set of agbnp_hip_execute_group whose shared launches the context's
                                            * last evaluation ran in (a group of one counts 1); 0 when it did not run through shared
                                            * launches */
  AGBNP_HIP_SCALAR_LAST_EVALUATION_KIND = 20,  /* how the last evaluation ENQUEUED on the context ran (valid without a completed
                                            * evaluation, like 15, 17, 18, 19 and 21): 0 a full evaluation, 1 an energy-only evaluation on
                                            * energy-only launches (alone or shared), 2 an energy-only request that ran as a full
                                            * evaluation with its forces sent to the context's own buffer, 3 a per-atom decomposition
                                            * (agbnp_hip_decompose_*), 4 a set-pair interaction matrix (agbnp_hip_pair_matrix_*),
                                            * 5 perturbation energies (agbnp_hip_perturbed_energies_*) */
  AGBNP_HIP_SCALAR_GROUP_BLOCK_WRITES = 21 /* how often the context's group argument blocks have been rewritten so far (one small
                                            * launch each); it stands still in a steady run of group calls with fixed position buffers */
};
/* the bits of AGBNP_HIP_SCALAR_OVERFLOW_KINDS */
enum agbnp_hip_overflow_kind {
  AGBNP_HIP_OVERFLOW_NODES = 1,            /* a subtree outgrew the store's nodes */
  AGBNP_HIP_OVERFLOW_ATOMS = 2,            /* ... its local atoms */
  AGBNP_HIP_OVERFLOW_PACKING = 4,          /* a forest packing mispredicted */
  AGBNP_HIP_OVERFLOW_ROW = 8,              /* a neighbour row outgrew its walk */
  AGBNP_HIP_OVERFLOW_REORDERED = 16,       /* the context reordered its atoms */
  AGBNP_HIP_OVERFLOW_FOREST_NODES = 32,    /* a forest of several work items outgrew its nodes */
  AGBNP_HIP_OVERFLOW_FOREST_ATOMS = 64,    /* ... its local atoms (the two kinds of AGBNP_HIP_OVERFLOW_PACKING) */
  AGBNP_HIP_OVERFLOW_SPLIT_PARTS = 256     /* bits 8..: times the part count of a lone work item that asked for its subtree to be
                                            * shared further */
};
/* vectors: length N, atom order */
enum agbnp_hip_vector {
  AGBNP_HIP_VECTOR_SELFVOL_VDW = 0,        /* self volume (vdW radii) */
  AGBNP_HIP_VECTOR_BORN = 1,               /* Born radius */
  AGBNP_HIP_VECTOR_SCALE = 2,              /* volume scaling factor */
  AGBNP_HIP_VECTOR_SELFVOL_LARGE = 3,      /* self volume (enlarged radii); only collected after agbnp_hip_set_diagnostics(ctx, 1) */
  AGBNP_HIP_VECTOR_SUBTREE_NODES = 4,      /* nodes and */
  AGBNP_HIP_VECTOR_SUBTREE_ATOMS = 5       /* local atoms of the overlap subtree rooted at the atom (tree shape, capacity planning) */
};
int agbnp_hip_set_diagnostics(agbnp_hip_context* ctx, int enabled); /* vector 3 is only collected when enabled */
int agbnp_hip_get_scalar(agbnp_hip_context* ctx, int which, double* value);
int agbnp_hip_get_vector(agbnp_hip_context* ctx, int which, double* out);

/* I4 lookup tables as uploaded (test support): sizes, then y/y2 [nscreened*nscreener*16] and per-atom types. */
int agbnp_hip_get_table_sizes(agbnp_hip_context* ctx, int* nscreened, int* nscreener);
int agbnp_hip_get_tables(agbnp_hip_context* ctx, double* y, double* y2, int* type_screened, int* type_screener);

/* Host-only table builder (no device needed; test support for the host logic): the radius typing and
 * the 16-node spline tables of AGBNPI42DLookupTable (openmmapi/src/AGBNPUtils.cpp:134-214).  y/y2 must hold
 * table_capacity doubles; fails with AGBNP_HIP_ERR_INVALID_ARGUMENT if nscreened*nscreener*16 exceeds it. */
int agbnp_hip_host_tables(int num_particles, const double* radius, const int* ishydrogen, int* nscreened, int* nscreener,
                          double* y, double* y2, int table_capacity, int* type_screened, int* type_screener);

/* Per-kernel timing (bench support).  When enabled, a hipEvent is recorded on the evaluation's stream in front
 * of every kernel; agbnp_hip_finish()/execute_host() turn them into accumulated milliseconds per kernel.
 * Enabling or disabling resets the accumulators.  total_ms / launches must hold agbnp_hip_num_kernels() items. */
int agbnp_hip_set_profiling(agbnp_hip_context* ctx, int enabled);
int agbnp_hip_num_kernels(void);
const char* agbnp_hip_kernel_name(int index);
int agbnp_hip_get_kernel_times(agbnp_hip_context* ctx, double* total_ms, long* launches);

int agbnp_hip_num_particles(const agbnp_hip_context* ctx);
int agbnp_hip_version(const agbnp_hip_context* ctx);

/* Message of the last error on this context; with ctx == NULL, of the last failed agbnp_hip_create() on the
 * calling thread (thread-local). */
const char* agbnp_hip_last_error(const agbnp_hip_context* ctx);

void agbnp_hip_destroy(agbnp_hip_context* ctx);

/* Number of HIP devices visible to this process (0 if none / runtime unavailable). */
int agbnp_hip_device_count(void);

/* What this library was built from: the first 16 hex digits of the SHA-256 of the engine's sources (csrc/Makefile), "unknown"
 * for a build made another way.  No counterpart in the reference; measurement support: scripts/profile_round.sh stores it
 * beside every rocprofv3 summary under profiles/, bench.py compares it with the library it is running (profile_head). */
const char* agbnp_hip_build_id(void);

#ifdef __cplusplus
}
#endif
#endif /* AGBNP_HIP_H_ */
