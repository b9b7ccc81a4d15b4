// Host engine + C ABI (include/agbnp_hip.h) of the gfx950 AGBNP force path: the context and what the engine's files share.
//
//   engine_setup.hip   a context's life: create, update_parameters, destroy; its device arrays and argument blocks
//   engine_eval.hip    one evaluation of one context: the request, its launches, the harvest, the single-context entry points
//   engine_group.hip   replica groups: the launches that several contexts share
//   engine_binding.hip binding-energy evaluations: three contexts behind one call, on top of the public group entry points
//   engine_report.hip  what a caller reads back: scalars, vectors, tables, kernel times, the diagnostic hooks
//
// Mirrors the life cycle of the reference's platform kernel
// (platforms/reference/src/ReferenceAGBNPKernels.cpp): initialize() :58-137 -> agbnp_hip_create,
// execute() :139-149 -> agbnp_hip_execute_{host,device}, copyParametersToContext() :1796-1815 ->
// agbnp_hip_update_parameters.  All device work of one evaluation is enqueued on one stream (enqueue_launch; the replica
// groups' shared launches: launch_set).  There is no CPU fallback: without a HIP device every entry point that computes fails
// with AGBNP_HIP_ERR_DEVICE.  No file of the host engine holds device code.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/agbnp_hip.h"
#include "adapter_kernels.h"
#include "agbnp_common.h"
#include "group_args.h"
#include "i4_tables.h"
#include "pair_kernels.h"
#include "tree_kernels.h"

using namespace agbnp;

// (what the engine's files share stays inside the library: the C ABI is its only boundary)
#define ENGINE_LOCAL __attribute__((visibility("hidden")))

template <class T>
struct ENGINE_LOCAL DevBuf {
  T* p = nullptr;
  size_t count = 0;
  // fill >= 0: every byte of the new array is set to it
  hipError_t alloc(size_t n, int fill = -1) {
    release();
    count = n;
    if (n == 0) return hipSuccess;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), n * sizeof(T));
    if (e != hipSuccess || fill < 0) return e;
    return hipMemset(p, fill, n * sizeof(T));
  }
  // Same size as before: the data is replaced IN PLACE and the device address stays what it was -- kernel
  // arguments frozen into a captured HIP graph keep pointing at live memory across agbnp_hip_update_parameters.
  hipError_t upload(const std::vector<T>& v) {
    if (p == nullptr || count != v.size()) {
      hipError_t e = alloc(v.size());
      if (e != hipSuccess) return e;
    }
    if (v.empty()) return hipSuccess;
    return hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    count = 0;
  }
  ~DevBuf() { release(); }
};

constexpr int kGlobalVariant = 4;  // the capacity variant whose store lives in HBM scratch (tree_kernels.hip, with_tree_variant: 0-3 in LDS)
constexpr int kGlobalGrid = 256;  // persistent workgroups of the global-scratch variant

// Engine settings from the environment, read once by agbnp_hip_create (a change takes effect in the next context).  "Used
// by" names bench.py and the GPU tests tests/test_gpu_{five_launches,healing,parity}.py by their last word.
//
//   AGBNP_HIP_...      default               values, clamp                                           used by
//   FIVE_LAUNCHES      on (versions 0, 1)    0: the k_prep launch stays                              bench.py, five_launches, healing, parity
//   ROWS               the row form          0: the tile kernels everywhere                          five_launches, parity
//   HEAL               on                    0: an overgrown forest voids the evaluation             healing, parity
//   SPLIT_FIT          on                    0: a lone subtree beyond the store climbs a variant     parity
//   GB_FAR             more than 8192 atoms  0 / 1: the far-strip test off / on                      parity
//   ROUND_PERMILLE     1000                  >= 100                                                  healing, parity
//   REPLAN_EVERY       16                    >= 1                                                    parity
//   ADAPTER_LAUNCH     off                   nonzero: execute_openmm through the adapter launch      parity
//   NO_PINNED_STAGING  unset                 set: pageable host-facing transfers                     parity
//   SKIN               0.1 nm                [0, 1]                                                  parity
//   ROW_MOVE           half the skin         >= 0, at most half the skin (0: rebuild every geometry) bench.py
//   ROW_SLICE          tuned on the device   > 0: fixed, [256, 512] in steps of 64                   parity
//   ROW_FILL           1.5                   >= 0.01                                                 parity
//   ROW_STRIDE         from the system       >= 128                                                  parity
//   MASK_SKIN          0.08 nm               [0, 0.5]                                                include/agbnp_hip.h documents it
//   GROUP_LAUNCHES     on                    0: the context runs alone inside agbnp_hip_execute_group    scripts/replica_group_timing.py
// SKIN and the ROW_* settings take effect only in a context that can run the row form (allocate_rows).
struct EngineSettings {
  bool five_launches = true;
  int rows = -1;    // -1: unset
  bool heal = true;
  bool split_fit = true;
  int gb_far = -1;  // -1: unset
  int round_permille = 1000;
  int replan_every = 16;
  bool adapter_launch = false;
  bool pinned_staging = true;
  double skin = 0.1;
  double row_move = -1.0;   // < 0: unset
  int row_slice = 0;        // 0: unset
  double row_fill = 1.5;    // the density bound behind the walked part of a list, in protein-interior densities
  int row_stride = 0;       // 0: unset
  bool group_launches = true;
  double mask_skin = 0.08;  // (0.06 and 0.08 cost the cavity launch the same; 0.04 renews the masks at every other evaluation of the headline's jitter)
};
ENGINE_LOCAL EngineSettings read_settings();  // (engine_setup.hip)

struct agbnp_hip_context {
  // ---- the system and the settings (engine_setup.hip)
  int n = 0, nh = 0, version = 1, method = 0, device = 0;
  double cutoff = 1.0;
  EngineSettings cfg;  // read_settings() at agbnp_hip_create
  std::string err;
  // host copies of the parameters (reference: ReferenceAGBNPKernels.h:60-91)
  std::vector<double> r_vdw, gamma, alpha, charge;
  std::vector<int> ish, a2h, h2a;
  I4TableSet lut;
  hipStream_t stream = nullptr;
  int cus = 256;
  int tree_slots[5] = {1280, 1024, 512, 256, 256};  // resident tree workgroups per variant (CUs x workgroups per CU by LDS)
  int slot_cap = 1024;  // work slots of the tree kernels: 4 x subtrees + resident workgroups of the smallest variant
  int mode = 0;  // AGBNP_HIP_MODE_* bits
  bool diagnostics = false;

  // ---- device arrays (engine_setup.hip).  An array that only the kernels read has no member here: it is named once, at its
  //      allocation, in the member of P or T it is written to (device_array), and `owned` frees it with the context.  The members below are what
  //      host code touches again: uploads in place, the reads of a harvest, regrowth, counts that are read back.
  std::vector<void*> owned;
  DevBuf<int> d_status, d_order, d_ftime, d_rows, d_forest, d_ctx_slot;
  DevBuf<double> d_charge, d_alpha;
  DevBuf<double> d_heavy;  // [kHvRows][hstride]: every per-heavy-atom double array of the tree and pair stages (tree_kernels.h)
                           // (five-launch mode: TWO such tables, see below)
  size_t hstride = 64;
  DevBuf<int2> d_sizes;
  DevBuf<double> d_egb_part, d_components;
  DevBuf<double> d_egb_rows;   // per-wave energy partials of the GB rows (the mode decides which of the two P.egb_part names)
  DevBuf<int> d_nl_flag;       // row form of the range-limited stages (pair_kernels.hip, k_rows): its flag block
  DevBuf<unsigned long long> d_node_pool;
  DevBuf<unsigned short> d_pair_pool;
  DevBuf<int> d_atom_pool;
  DevBuf<char> d_scratch;
  int variant = 0;
  bool rows_capable = false;   // the row form's arrays exist
  bool rows_disabled = false;  // a neighbour row outgrew its stride once: the tile kernels from then on
  int row_boost = 1;           // widens the part of a list that the row launches walk (doubles when a list has outgrown it)
  // AGBNP_HIP_SKIN (nm), AGBNP_HIP_ROW_MOVE (nm; < 0: half the skin), AGBNP_HIP_ROW_SLICE (entries per slice, fixed; 0: tuned on
  // the device, see rows_close_evaluation).  Mirrors of cfg that allocate_rows fills, NOT cfg itself: a context that cannot run the
  // row form keeps these defaults whatever the environment says, and nl_build2, nlg_build2, nl_move2 and row_target of its
  // argument block come from them (AGBNP_HIP_ROW_FILL has no mirror: without rows every walked length is capped at 1)
  double skin = 0.1, row_move = -1.0;
  int row_slice = 0;
  // ---- five-launch mode (the default for version 1 since round 5; AGBNP_HIP_FIVE_LAUNCHES=0 keeps the k_prep launch; the LDS
  //      stores (variants 0-3), the FP64 row form of the pair stages; the caller's FP64 [3n] positions or -- round 6 -- an OpenMM context's
  //      posq; inside stream captures the device names the evaluation's set): no k_prep launch.  The trailing workgroups of the
  //      cavity launch do k_prep's per-atom work; what the tree launch needs clean BEFORE it starts -- its accumulators, the
  //      subtree shapes, the per-evaluation status words -- exists twice and alternates with the evaluation's parity (the
  //      trailing workgroups clear the other set); the tree reads the caller's positions itself; the level-2 neighbour masks
  //      carry a skin and are laid down anew ON THE DEVICE, by tiles at the tail of the Born-rows launch, when a heavy atom has
  //      used a quarter of it (beyond half the evaluation is void: a jump of more than 0.04 nm costs one withheld evaluation,
  //      include/agbnp_hip.h); a launch of their own (k_masks) lays them down for a fresh context and after an OpenMM context
  //      has reordered its atoms
  bool five = false;           // asked for
  bool five_active = false;    // ... and in effect (switched off for good by the HBM-resident store of variant 4, pair stages other than the FP64 row form, the diagnostic pass-1 self volumes)
  int parity = 0;              // of the evaluation whose results the device holds (read back at every harvest)
  int five_evals = 0;          // evaluations enqueued in the mode so far: evaluation k works on set k & 1
  bool five_device = false;    // the device names the set (from the context's first stream capture on: see PairArgs::five)
  bool masks_valid = false;
  DevBuf<int> d_estatus, d_row_atoms;
  int row_atoms_kind = 0;       // five-launch mode: what d_row_atoms holds for the packing in use -- 0 atom indices (the caller's
                                // [3n] positions), 1 slots of an OpenMM context's order (posq), -1 stale (the context reordered);
                                // changed through set_row_atoms_kind only
  size_t nhp() const { return (size_t)std::max(nh, 1); }  // heavy atoms, or the one entry that arrays by heavy index have without any
  int tables() const { return five ? 2 : 1; }             // sets of {heavy-atom table, subtree shapes}
  int set_held() const { return five_active ? parity : 0; }  // the set that holds the last evaluation's results
  double* htable(int p) const { return d_heavy.p + (size_t)p * kHvRows * hstride; }
  double* hrow(int r) const { return htable(set_held()) + (size_t)r * hstride; }
  int2* sizes(int p) const { return d_sizes.p + (size_t)p * nhp(); }
  PairArgs P{};
  TreeArgs T{};
  unsigned generation = 1;     // bumped whenever kernel arguments a captured graph has frozen go stale
  int fallback_parts = 1;      // the packing an overflowed evaluation is repeated on: every subtree shared among this many work items, each
                               // alone in its slot (1, or 4 once a lone item has outgrown the store; never lowered)

  // ---- evaluations (engine_eval.hip)
  // host-API staging
  DevBuf<double> d_pos_in, d_force_tmp, d_energy_tmp;
  std::vector<double> h_force_tmp;
  // energy-only evaluations (agbnp_hip_energy_*): where the forces of one that runs as a full evaluation go (the fallback,
  // energy_only_fast) -- [3n] FP64 for agbnp_hip_energy_device, fixed-point planes [3 padded] for agbnp_hip_energy_openmm
  // (energy_role routes the energy to an OpenMM accumulator only beside a fixed-point force target); never read
  DevBuf<double> d_eo_force;
  DevBuf<unsigned long long> d_eo_fixed;
  // per-atom decompositions and set-pair matrices (agbnp_hip_decompose_host, agbnp_hip_pair_matrix_host): the four planes or the
  // matrix, and the energy behind them, [4n + 1] or [S S + 1], on the device and on the host
  DevBuf<double> d_decomp;
  std::vector<double> h_decomp;
  // the partition of agbnp_hip_set_atom_sets as the matrix launch reads it (pair_kernels.h, AtomSets: sets.num_sets == 0: none
  // set).  No evaluation reads it; agbnp_hip_update_parameters leaves it alone
  DevBuf<unsigned char> d_set_rank;
  DevBuf<int> d_set_lists, d_set_counts;
  AtomSets sets;
  // the parameter sets of agbnp_hip_set_parameter_sets as the perturbation launch reads them (pair_kernels.h, ParamSets: three [M][n]
  // tables; psets.num_sets == 0: none set).  No evaluation reads them; agbnp_hip_update_parameters leaves them alone
  DevBuf<double> d_pset_nu, d_pset_alpha, d_pset_charge;
  ParamSets psets;
  int forests_hint = 0;        // forests of the last evaluation the host has read the status of (0: none yet); reset by a fallback packing
  std::vector<int> withheld;   // evaluations (numbered from the previous finish) that the last finish found withheld
  int withheld_count = 0;
  std::vector<int> carried;     // withheld evaluations of execute_device harvested by an execute_host call in between (see there)
  int carried_count = 0, carried_seq = 0;
  bool unfinished = false;      // evaluations enqueued by execute_device / execute_openmm since the last finish
  int enqueued = 0;             // ... how many: what agbnp_hip_wait_verdict waits for (the device numbers them the same way)
  int* h_status = nullptr;      // pinned, mapped: {evaluations completed, withheld} since the last finish (agbnp_hip_poll)
  // what harvest() reads of the device: asynchronous copies in front of ONE stream synchronisation.  With the pinned staging
  // of the host-facing paths the report lives in pinned memory (h_report), without it (AGBNP_HIP_NO_PINNED_STAGING) in the
  // context (own_report); execute_host's positions, forces and energy travel through h_xfer ([3n] in, [3n + 1] out) instead
  // of pageable memory
  struct HostReport {
    int status[kStatTotalWords];
    double components[4];
    int rows[kNlReported], pack[kPsReported];
    int five[2 * kStatBlockStride];  // five-launch mode: the two blocks of per-evaluation status words ...
    int epoch;                       // ... and the device's evaluation counter
  };
  HostReport* h_report = nullptr;
  HostReport own_report{};
  double* h_xfer = nullptr;
  // agbnp_hip_execute_host's short cut: an evaluation that the pinned status words call complete skips the reads of the
  // device (they are diagnostics) and leaves the log running; the reads are caught up with when somebody asks for a
  // diagnostic, when an evaluation is enqueued through a device-resident entry point, and every 1024 evaluations
  int lazy_evals = 0;           // evaluations of execute_host since the log was last read and cleared: the FIRST entries of the
                                // running log (a device-resident entry point that follows counts on from there; nothing is
                                // synchronised for the hand-over, so it is safe inside a graph capture)
  int last_device_seq = 0;      // harvest(): evaluations of the device-resident entry points that the log just read held
  std::vector<void*> user_streams;  // streams the caller has enqueued on since the last finish (drained before parameters change)
  // agbnp_hip_execute_openmm without an adapter launch: k_prep reads the context's posq through the particle -> slot and heavy
  // index -> slot maps (d_ctx_slot, d_hslot), built for the atomIndex array at order_ptr and checked on the device in every
  // evaluation; a context that has reordered its atoms voids ONE evaluation (kStatOrderStale), the maps are rebuilt, the
  // caller repeats (AGBNP_HIP_ADAPTER_LAUNCH=1: the adapter launch of rounds 1-2 instead)
  DevBuf<int> d_hslot;
  bool order_valid = false;
  const int* order_ptr = nullptr;
  bool jump_expected = false;        // agbnp_hip_expect_jump: the next evaluation lays the neighbour masks down at its own positions first

  // ---- replica groups (engine_group.hip; agbnp_hip_execute_group): the context's argument blocks of the shared launches, one per
  //      parity of the five-launch mode's sets, and what was last written to each (a block is rewritten only when it changes)
  DevBuf<GroupMemberArgs> d_group;
  GroupMemberArgs group_written[2];
  bool group_valid[2] = {false, false};
  hipEvent_t group_event = nullptr;  // joins the context's own stream and a group's stream
  int group_members = 0;             // scalar 19: members of the launch set the last evaluation shared (0: it ran alone)
  int group_block_writes = 0;        // scalar 21: k_group_put launches so far
  int last_kind = 0;                 // scalar 20: 0 a full evaluation, 1 energy-only on energy-only launches, 2 energy-only run as a full one,
                                     // 3 a per-atom decomposition, 4 a set-pair interaction matrix, 5 perturbation energies

  // ---- what the last harvest read (engine_report.hip reads it back to the caller)
  Timeline timeline;
  double kernel_ms[kKernelCount] = {0};
  long kernel_launches[kKernelCount] = {0};
  int last_status[kStatTotalWords] = {0};
  double last_components[4] = {0, 0, 0, 0};
  int last_pack[kPsReported] = {0};  // the forest packing's words up to kPsPlans (PackStateWord) as of the last harvest
  int last_rows[kNlReported] = {0};  // the row-flag block's words up to kNlSlice (RowFlagWord) as of the last harvest
  bool have_results = false;

  int fail(int code, const std::string& msg) {
    err = msg;
    return code;
  }
  int hipfail(hipError_t e, const char* what) {
    err = std::string(what) + ": " + hipGetErrorString(e);
    return AGBNP_HIP_ERR_DEVICE;
  }
  ~agbnp_hip_context() {  // (agbnp_hip_destroy, and an agbnp_hip_create that fails half-way)
    for (void* p : owned) (void)hipFree(p);
  }
};

#define HIP_TRY(ctx, call)                                  \
  do {                                                      \
    hipError_t e__ = (call);                                \
    if (e__ != hipSuccess) return (ctx)->hipfail(e__, #call); \
  } while (0)

// A device array that only the kernels read: n elements, every byte set to `fill` (< 0: left as allocated), owned by the
// context until agbnp_hip_destroy deletes it.  *out is the member of P or T that names it (null for n == 0).
template <class T>
ENGINE_LOCAL hipError_t device_array(agbnp_hip_context* c, T** out, size_t n, int fill = -1) {
  *out = nullptr;
  if (n == 0) return hipSuccess;
  void* p = nullptr;
  hipError_t e = hipMalloc(&p, n * sizeof(T));
  if (e != hipSuccess) return e;
  c->owned.push_back(p);
  *out = static_cast<T*>(p);
  return fill < 0 ? hipSuccess : hipMemset(p, fill, n * sizeof(T));
}
// ... filled from the host
template <class T>
ENGINE_LOCAL hipError_t device_array(agbnp_hip_context* c, T** out, const std::vector<std::remove_const_t<T>>& v) {
  hipError_t e = device_array(c, out, v.size());
  if (e != hipSuccess || v.empty()) return e;
  return hipMemcpy(c->owned.back(), v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
}

inline int row_groups(int atoms) { return (atoms + kRowGroup - 1) / kRowGroup; }  // groups of row atoms that share a neighbour list

// ---- engine_setup.hip
extern ENGINE_LOCAL thread_local std::string g_create_error;  // message of the last failed agbnp_hip_create / host_tables on THIS thread
ENGINE_LOCAL int ensure_scratch(agbnp_hip_context* c);
ENGINE_LOCAL int upload_identity_packing(agbnp_hip_context* c);
ENGINE_LOCAL void apply_parity(agbnp_hip_context* c);
ENGINE_LOCAL void derive_args(agbnp_hip_context* c);
ENGINE_LOCAL int mark_rows_stale(agbnp_hip_context* c);

// ---- engine_eval.hip
// What a caller asks of one evaluation.  It is written into the argument blocks by bind_request (inside enqueue_prepare) and taken
// out again by Unbind, on every return path of enqueue / group_enqueue: between evaluations P and T name no caller's buffer to clear
// and no OpenMM context.
// An analysis (agbnp_hip_decompose_*, agbnp_hip_pair_matrix_*, agbnp_hip_perturbed_energies_*, a group's member) is a property of the request: ONE
// evaluation in the context's overflow log -- the energy-only evaluation of the context (energy_only_fast: its four / two launches;
// elsewhere the full evaluation with its forces sent to d_eo_force) with the cavity launch's instantiation that also collects the
// enlarged-radius self volumes (sv_large(): row kHvSvLarge) -- and behind it, on the same stream, the one launch that adds to the
// caller's target: the four planes (k_decompose, decompose_kernels.hip; a launch set's members share k_group_decompose) or, with a
// partition set, the set-pair interaction matrix (k_pair_matrix), or, with parameter sets set, the energies under those sets
// (k_perturb, perturb_kernels.hip) -- one of the three.  enqueue_launch makes that launch and names the
// kind in last_kind; launch_set makes the shared one.  The energy leaves with the evaluation's own energy role (energy_request:
// no energy word: into the context's spare word), the target is gated on the same verdict words.  Nothing of the context's state
// differs from what the evaluation alone leaves: the request selects the instantiation, c->diagnostics is not touched.
// fast+single: the terms are FP64 (header), so the evaluation runs with the single-precision option lifted for this call
// (LiftSingle) -- the same lists and masks (the reach is the fast mode's), other pair-term arithmetic; kernel arguments travel by
// value, so nothing enqueued before or after is affected.
enum class Analysis { none, planes, matrix, perturb };
struct EvalRequest {
  const double* pos = nullptr;   // [3n] FP64 positions on the device
  double* force = nullptr;       // [3n] FP64 forces, added to (energy-only: where a full evaluation's would go, d_eo_force)
  double* energy = nullptr;      // [1]
  hipStream_t stream = nullptr;
  bool energy_only = false;
  Analysis analysis = Analysis::none;  // what follows the evaluation, and ...
  double* target = nullptr;      // ... what it adds to: the planes [4][n], the matrix [S][S] or the energies [M]
  double* zero_out = nullptr;    // the host entry points' staging buffer, cleared first (PairArgs::zero_out)
  OpenmmSource in;               // agbnp_hip_execute_openmm / agbnp_hip_energy_openmm: the context's posq ...
  OpenmmTargets omm;             // ... and its fixed-point planes and energy accumulator
  bool sv_large() const { return analysis != Analysis::none; }  // an analysis is exactly what needs the enlarged-radius self volumes
};
struct ENGINE_LOCAL Unbind {
  agbnp_hip_context* const* ctxs;
  int count;
  ~Unbind();
};
// The requests that carry an analysis in the fast+single mode: the option is off from before the member's enqueue_prepare
// (host_set_only there reads P.single) until its request has left the argument blocks -- declared in front of the Unbind, destroyed
// behind it.  The generation is not touched: the mode is what it was when the call returns.
struct ENGINE_LOCAL LiftSingle {
  agbnp_hip_context* lifted[kMaxGroup];
  int count = 0;
  void lift(agbnp_hip_context* c, const EvalRequest& r) {
    if (!r.sv_large() || !(c->mode & AGBNP_HIP_MODE_SINGLE)) return;
    c->mode &= ~AGBNP_HIP_MODE_SINGLE;
    derive_args(c);
    lifted[count++] = c;
  }
  ~LiftSingle() {
    for (int i = 0; i < count; i++) {
      lifted[i]->mode |= AGBNP_HIP_MODE_SINGLE;
      derive_args(lifted[i]);
    }
  }
};
// What enqueue() decides before its launches (enqueue_prepare) and hands to them (enqueue_launch)
struct EvalPlan {
  int tree_grid = 1;   // workgroups of the tree launches
  bool fused = false;  // version 1: the forces leave with the pseudo-volume launch
};
ENGINE_LOCAL int enter(agbnp_hip_context* c, void* stream, hipStream_t* st);
ENGINE_LOCAL bool is_capturing(hipStream_t st);
ENGINE_LOCAL void note_stream(agbnp_hip_context* c, void* stream);
ENGINE_LOCAL void set_row_atoms_kind(agbnp_hip_context* c, int kind);
ENGINE_LOCAL bool energy_only_fast(const agbnp_hip_context* c);
ENGINE_LOCAL int enqueue_prepare(agbnp_hip_context* c, const EvalRequest& r, EvalPlan& plan);
ENGINE_LOCAL void set_outputs(agbnp_hip_context* c, double* d_force, bool fused);
ENGINE_LOCAL int enqueue_launch(agbnp_hip_context* c, const EvalPlan& plan, const EvalRequest& r);
ENGINE_LOCAL int harvest(agbnp_hip_context* c, int* repeat, hipStream_t st);
ENGINE_LOCAL int catch_up(agbnp_hip_context* c);
ENGINE_LOCAL int carry_unfinished(agbnp_hip_context* c);
ENGINE_LOCAL int host_evaluation(agbnp_hip_context* c, const double* pos, double* forces, double* energy);
ENGINE_LOCAL int host_decomposition(agbnp_hip_context* c, const double* pos, double* per_atom, double* energy);
// the energy-only request with its analysis (d_energy null: the context's spare word); a host form's analysis through d_decomp [count + 1]
ENGINE_LOCAL EvalRequest energy_request(agbnp_hip_context* c, const double* d_pos, double* d_energy, hipStream_t st, Analysis kind = Analysis::none, double* target = nullptr);
ENGINE_LOCAL int stage_analysis(agbnp_hip_context* c, const double* pos, Analysis kind, size_t count, hipStream_t st, EvalRequest* r);
ENGINE_LOCAL hipError_t fetch_analysis(agbnp_hip_context* c, size_t count, hipStream_t st);
ENGINE_LOCAL void deliver_analysis(const agbnp_hip_context* c, size_t count, double* out, double* energy);

// ---- engine_group.hip (what replica groups and binding groups both need)
ENGINE_LOCAL bool spans_overlap(const double* a, size_t na, const double* b, size_t nb);  // two output spans; a null one overlaps nothing
ENGINE_LOCAL hipError_t join_streams(hipEvent_t& event, hipStream_t from, hipStream_t to);
