// Replica groups (engine_context.h; agbnp_hip_execute_group, group_args.h): the evaluations of several contexts on one set of launches.
// The five kinds of group call -- full, energy-only, decomposition, pair matrix, perturbation -- are one description (GroupCall), one check, one device form
// and one host form; what a kind does differently is in the requests it builds and in the host form's three named steps.
#include "engine_context.h"

// (shared with the binding groups, engine_binding.hip, whose output pointers may be null: a null span overlaps nothing)
bool spans_overlap(const double* a, size_t na, const double* b, size_t nb) { return a && b && a < b + nb && b < a + na; }

// joins two streams through `event` (made on first use): `to` waits for what is on `from` now
hipError_t join_streams(hipEvent_t& event, hipStream_t from, hipStream_t to) {
  if (from == to) return hipSuccess;
  hipError_t e = event ? hipSuccess : hipEventCreateWithFlags(&event, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventRecord(event, from);
  if (e == hipSuccess) e = hipStreamWaitEvent(to, event, 0);
  return e;
}

namespace {
// A member shares the launches of its launch set when its evaluation is exactly the default launch sequence: the five-launch
// mode with the host-named set, the Reference semantics and (version 1) the FP64 row form, an LDS-resident capacity variant, the
// forces leaving with the pseudo-volume launch, no diagnostics, no profiling.  Every other member runs its own launches.
// (An energy-only group makes no pseudo-volume launch: the condition on the forces does not apply there.)
bool group_shares(const agbnp_hip_context* c, const EvalPlan& plan, const EvalRequest& r) {
  if (!c->cfg.group_launches || c->timeline.enabled || !energy_only_fast(c)) return false;
  if (r.in.posq || r.omm.force_fixed || c->P.five != 1) return false;
  return c->version == 0 || plan.fused || r.energy_only;
}

// A group call: its kind, and the buffers its entry point was given.  host: the host form -- positions, forces and planes are host
// arrays and the energies come back in `energies`; the device form has one energy word per member in d_energies.
enum class GroupKind { full, energy_only, decomposition, matrix, perturb };
struct GroupCall {
  GroupKind kind;
  const char* who;
  bool host;
  const double* const* pos;  // every kind
  double* const* forces;     // a full call's, [3n] per member
  double* const* planes;     // a decomposition's, [4n] per member; a pair-matrix call's matrices, [S_m S_m] per member; a
                             // perturbation call's energies under the member's sets, [M_m] per member
  double* const* d_energies;
  double* energies;
};

// the analysis that a kind's requests carry
Analysis analysis_of(GroupKind kind) {
  return kind == GroupKind::perturb ? Analysis::perturb : kind == GroupKind::matrix ? Analysis::matrix : kind == GroupKind::decomposition ? Analysis::planes : Analysis::none;
}
bool is_analysis(GroupKind kind) { return analysis_of(kind) != Analysis::none; }

// words of a member's analysis target: the four planes, the matrix of its own partition, or one energy per set of its own
size_t target_words(const agbnp_hip_context* c, GroupKind kind) {
  const size_t S = (size_t)c->sets.num_sets;
  return kind == GroupKind::perturb ? (size_t)c->psets.num_sets : kind == GroupKind::matrix ? S * S : 4 * (size_t)c->n;
}

// The arguments of a group call, checked before anything is launched or changed.  Every kind needs positions, a full call forces,
// a decomposition planes, a pair-matrix call matrices -- and a partition in every member --, a perturbation call energy words [M_m]
// -- and parameter sets in every member; the energies are the host form's array or the device form's words, which the analyses
// alone may leave out altogether.  The device form's outputs -- energy words,
// force buffers [3n], plane buffers [4n], matrices [S_m S_m] -- must not overlap those of another member; the planes' and the
// matrices' clashes, with one another or with an energy word, are said in a message of their own.
int check_group(agbnp_hip_context* const* ctxs, int count, const GroupCall& g) {
  const char* const who = g.who;
  if (!ctxs || count < 1 || count > kMaxGroup) {
    if (ctxs && count >= 1 && ctxs[0]) ctxs[0]->fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, std::string(who) + ": a group has 1 to 16 members");
    return AGBNP_HIP_ERR_INVALID_ARGUMENT;
  }
  for (int i = 0; i < count; i++)
    if (!ctxs[i]) return AGBNP_HIP_ERR_INVALID_ARGUMENT;
  agbnp_hip_context* c0 = ctxs[0];
  const bool full = g.kind == GroupKind::full, matrix = g.kind == GroupKind::matrix, perturb = g.kind == GroupKind::perturb;
  const bool analysis = is_analysis(g.kind);
  const std::string clash_message = std::string(who) + (perturb  ? ": energy arrays of two members overlap"
                                                        : matrix ? ": matrices of two members overlap"
                                                                 : ": plane buffers of two members overlap");
  // (what this kind and form read of the description; null below: not theirs)
  const double* const* pos = g.pos;
  double* const* forces = full ? g.forces : nullptr;
  double* const* planes = analysis ? g.planes : nullptr;
  double* const* d_energies = g.host ? nullptr : g.d_energies;
  if (!pos || (full && !forces) || (analysis && !planes) || (g.host ? !g.energies : !d_energies && !analysis))
    return c0->fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, std::string(who) + ": null pointer");
  for (int i = 0; i < count; i++) {
    if (ctxs[i]->device != c0->device) return c0->fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, std::string(who) + ": members on different devices");
    for (int j = 0; j < i; j++)
      if (ctxs[j] == ctxs[i]) return c0->fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, std::string(who) + ": the same context twice");
  }
  for (int i = 0; i < count && matrix; i++)
    if (ctxs[i]->sets.num_sets < 1)
      return c0->fail(AGBNP_HIP_ERR_INVALID_ARGUMENT,
                      std::string(who) + ": member " + std::to_string(i) + ": no partition has been set (agbnp_hip_set_atom_sets)");
  for (int i = 0; i < count && perturb; i++)
    if (ctxs[i]->psets.num_sets < 1)
      return c0->fail(AGBNP_HIP_ERR_INVALID_ARGUMENT,
                      std::string(who) + ": member " + std::to_string(i) + ": no parameter sets have been set (agbnp_hip_set_parameter_sets)");
  for (int i = 0; i < count; i++) {
    if (!pos[i] || (forces && !forces[i]) || (d_energies && !d_energies[i]) || (planes && !planes[i]))
      return c0->fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, std::string(who) + ": null pointer");
    // (the host form's targets are host arrays, each OVERWRITTEN by its own member's result: they are held to the same rule)
    for (int j = 0; j < i && planes; j++) {
      const size_t ni = target_words(ctxs[i], g.kind), nj = target_words(ctxs[j], g.kind);
      bool clash = spans_overlap(planes[i], ni, planes[j], nj);
      if (d_energies) clash = clash || spans_overlap(planes[i], ni, d_energies[j], 1) || spans_overlap(d_energies[i], 1, planes[j], nj);
      if (clash) return c0->fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, clash_message);
    }
    // (a member's own energy word inside its own planes or matrix)
    if (planes && d_energies && spans_overlap(planes[i], target_words(ctxs[i], g.kind), d_energies[i], 1))
      return c0->fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, clash_message);
    for (int j = 0; j < i && d_energies; j++) {
      const size_t ni = 3 * (size_t)ctxs[i]->n, nj = 3 * (size_t)ctxs[j]->n;
      bool clash = spans_overlap(d_energies[i], 1, d_energies[j], 1);
      if (forces)
        clash = clash || spans_overlap(forces[i], ni, forces[j], nj) || spans_overlap(forces[i], ni, d_energies[j], 1) ||
                spans_overlap(d_energies[i], 1, forces[j], nj);
      if (clash)
        return c0->fail(AGBNP_HIP_ERR_INVALID_ARGUMENT,
                        std::string(who) + (forces ? ": output buffers of two members overlap" : ": energy words of two members overlap"));
    }
  }
  return AGBNP_HIP_OK;
}

// One launch per stage for the members set[0..m) of a launch set (same version, capacity variant and far-strip test; one kind of
// request).  Energy-only (agbnp_hip_energy_group): version 1 FOUR launches -- cavity, Born rows, the GB stage's energy-only
// instantiation, the three role workgroups per member --, version 0 the cavity launch and the output launch in its force-less
// shape.  Both kinds of call build the SAME argument block for a member's parity (the block holds no output pointer, and what
// the energy-only launches read of it a full call fills too), so a run that mixes them rewrites nothing.
// A decomposition group (agbnp_hip_decompose_group; the requests carry the planes as their analysis) is an energy-only set whose cavity
// launch is the instantiation that also collects the enlarged-radius self volumes, with ONE more launch behind it: the planes of
// every member (decompose_kernels.hip: k_group_decompose; FIVE launches, version 0 three).  The same blocks again.
// A pair-matrix group (agbnp_hip_pair_matrix_group; the requests carry the matrices) is the same set with the matrix launch of every
// member in the place of the plane launch (pair_matrix_kernels.hip: k_group_pair_matrix), on the same grids; the members'
// partitions and matrix pointers travel in that launch's argument (GroupMatrices), so the blocks are the same once more.
// A perturbation group (agbnp_hip_perturbed_energies_group) likewise, with the perturbation launch of every member in that place
// (perturb_kernels.hip: k_group_perturb; the members' tables and output words in GroupPerturb).
int launch_set(agbnp_hip_context* const* ctxs, const int* set, int m, const EvalPlan* plans, const EvalRequest* reqs) {
  const bool energy_only = reqs[set[0]].energy_only, decomposition = reqs[set[0]].sv_large();  // (either analysis)
  const bool matrix = reqs[set[0]].analysis == Analysis::matrix, perturb = reqs[set[0]].analysis == Analysis::perturb;
  const hipStream_t st = reqs[set[0]].stream;
  agbnp_hip_context* const c0 = ctxs[set[0]];
  const int version = c0->version, variant = c0->variant;
  // version 1: cavity, Born rows, GB tiles, chain-rule rows, pseudo volumes (energy-only: cavity, Born rows, GB tiles, roles); 0: cavity, outputs
  const int stages = version == 1 ? (energy_only ? 4 : 5) : 2;
  GroupLaunch G[5], Gplanes;  // (Gplanes: the plane or matrix launch of an analysis group, behind the energy-only stages)
  GroupOutputs out;
  GroupPlanes planes;
  GroupMatrices matrices;
  GroupPerturb perturbed;
  size_t matrix_lds = 0;
  std::memset(G, 0, sizeof(G));
  std::memset(&Gplanes, 0, sizeof(Gplanes));
  std::memset(&out, 0, sizeof(out));
  std::memset(&planes, 0, sizeof(planes));
  std::memset(&matrices, 0, sizeof(matrices));
  std::memset(&perturbed, 0, sizeof(perturbed));
  size_t lds[5] = {tree_variant_lds_bytes(variant), 0, 0, 0, tree_variant_replay_bytes(variant)};
  for (int k = 0; k < m; k++) {
    const int i = set[k];
    agbnp_hip_context* const c = ctxs[i];
    const EvalPlan& plan = plans[i];
    // (the block's copy carries no force pointer; an energy-only set makes no pseudo-volume launch: no force target at all)
    if (version == 1) set_outputs(c, energy_only ? nullptr : reqs[i].force, true);
    GroupMemberArgs a;
    std::memset(&a, 0, sizeof(a));
    a.P = c->P;
    a.T = c->T;
    // (the replay's weights; whatever the kind of request, so that the blocks stay the same: a set without a replay does not read it)
    a.T.single_gather = tree_single_gather(variant, version) ? 1 : 0;
    a.T.out.forest_blocks = plan.tree_grid;
    a.T.out.force = nullptr;  // (the caller's outputs travel in the launch argument: the block stays what it was)
    a.components = c->d_components.p;
    a.tree_blocks = plan.tree_grid;
    a.pseudo_blocks = version == 1 ? tree_pseudo_grid(variant, kGlobalGrid, plan.tree_grid, a.T) : 0;
    // the member's grids and LDS exactly as its own launches would take them (enqueue_launch): from pair_launch_shape and the
    // tree_*_grid functions, which size those too
    const PairLaunchShape sh = pair_launch_shape(c->P, version);
    if (version == 1) {
      a.born_role = sh.born_mask_from;
      a.chain_role = (int)sh.chain_lds;
    } else {
      a.out_role_bytes = sh.out_masks.role_bytes;
      a.out_mask_from = sh.out_masks.mask_from;
    }
    // the block of this evaluation's set, rewritten in stream order where it changed
    const int p = (c->five_evals - 1) & 1;
    if (c->d_group.p == nullptr) HIP_TRY(c, c->d_group.alloc(2));
    if (!c->group_valid[p] || std::memcmp(&c->group_written[p], &a, sizeof(a)) != 0) {
      HIP_TRY(c, launch_group_put(a, c->d_group.p + p, st));
      std::memcpy(&c->group_written[p], &a, sizeof(a));
      c->group_valid[p] = true;
      c->group_block_writes++;
    }
    const unsigned long long addr = (unsigned long long)(uintptr_t)(c->d_group.p + p);
    // (energy-only: the roles launch in place of the chain-rule launch; version 0: the output launch in its force-less shape)
    const int cavity_blocks = tree_five_grid(plan.tree_grid, c->P);
    const int grid1[5] = {cavity_blocks, sh.born_blocks, sh.gb_tile_blocks, energy_only ? sh.role_blocks : sh.chain_blocks, a.pseudo_blocks};
    const int grid0[2] = {cavity_blocks, energy_only ? sh.out_energy.blocks : sh.out_masks.blocks};
    for (int s = 0; s < stages; s++) {
      G[s].first[k + 1] = G[s].first[k] + (version == 1 ? grid1[s] : grid0[s]);
      G[s].args[k] = addr;
    }
    out.force[k] = energy_only ? 0ull : (unsigned long long)(uintptr_t)reqs[i].force;
    out.energy[k] = (unsigned long long)(uintptr_t)reqs[i].energy;
    Gplanes.first[k + 1] = Gplanes.first[k] + decompose_blocks(c->n, version);
    Gplanes.args[k] = addr;
    planes.per_atom[k] = (unsigned long long)(uintptr_t)reqs[i].target;
    if (matrix) {
      matrices.sets[k] = c->sets;
      matrices.matrix[k] = planes.per_atom[k];
      matrix_lds = std::max(matrix_lds, sizeof(double) * (size_t)c->sets.depth * (size_t)c->sets.depth);
    }
    if (perturb) {
      perturbed.sets[k] = c->psets;
      perturbed.energies[k] = planes.per_atom[k];
    }
    if (version == 1) {
      lds[1] = std::max(lds[1], sh.born_lds);
      lds[3] = std::max(lds[3], sh.chain_lds);
    } else {
      lds[1] = std::max(lds[1], (size_t)sh.out_masks.role_bytes);
    }
    c->group_members = m;
    c->last_kind = perturb ? 5 : matrix ? 4 : decomposition ? 3 : energy_only ? 1 : 0;
  }
  for (int s = 0; s < stages; s++) G[s].count = m;
  Gplanes.count = m;
  // the launch behind an analysis set's energy-only stages: the members' energies under their sets, their matrices, or their planes
  auto analysis = [&]() -> hipError_t {
    if (perturb) return launch_group_perturb(Gplanes, perturbed, version, st);
    return matrix ? launch_group_pair_matrix(Gplanes, matrices, version, matrix_lds, st) : launch_group_decompose(Gplanes, planes, version, st);
  };
  // (an analysis set collects the self volumes of pass 1 and has no replay: both gathers)
  HIP_TRY(c0, launch_group_cavity_five(variant, G[0], lds[0], st, decomposition, tree_single_gather(variant, version) && !decomposition));
  if (version == 0) {
    if (energy_only)
      HIP_TRY(c0, launch_group_outputs_energy(G[1], out, lds[1], st));
    else
      HIP_TRY(c0, launch_group_outputs(G[1], out, lds[1], st));
    if (decomposition) HIP_TRY(c0, analysis());
    return AGBNP_HIP_OK;
  }
  HIP_TRY(c0, launch_group_born_rows(G[1], lds[1], st));
  if (energy_only) {
    HIP_TRY(c0, launch_group_gb_energy(c0->P.gb_far, G[2], st));
    HIP_TRY(c0, launch_group_energy_roles(G[3], out, lds[3], st));
    if (decomposition) HIP_TRY(c0, analysis());
    return AGBNP_HIP_OK;
  }
  HIP_TRY(c0, launch_group_gb(c0->P.gb_far, G[2], st));
  HIP_TRY(c0, launch_group_chain_rows(G[3], out, lds[3], st));
  HIP_TRY(c0, launch_group_pseudo(variant, G[4], out, lds[4], st));
  return AGBNP_HIP_OK;
}

// every member's evaluation (one request each, all of one kind and on one stream): the per-evaluation host logic of each, then one
// launch per stage and launch set, then the members that run alone.  When something fails, the members whose launches were not
// reached get back the counts their enqueue_prepare advanced (enqueue index, five-launch set parity), so that host and device keep
// counting alike; a member whose launches failed half-way is in the state a failed agbnp_hip_execute_device leaves
// (AGBNP_HIP_ERR_DEVICE: recreate it).  A member that does not share runs what its own entry point would run for its request.
// A decomposition group's member that runs alone -- by itself or as a launch set of one -- runs what agbnp_hip_decompose_device runs
// for it: enqueue_launch makes its own plane launch; fast+single with the single-precision option lifted for this call (LiftSingle).
int group_enqueue(agbnp_hip_context* const* ctxs, int count, const EvalRequest* reqs) {
  LiftSingle single;
  const Unbind unbind{ctxs, count};
  EvalPlan plans[kMaxGroup];
  bool shares[kMaxGroup], done[kMaxGroup], launched[kMaxGroup] = {};
  int was_enqueued[kMaxGroup], was_five_evals[kMaxGroup], prepared = 0;
  auto undo = [&](int rc) {
    for (int i = 0; i < prepared; i++)
      if (!launched[i]) ctxs[i]->enqueued = was_enqueued[i], ctxs[i]->five_evals = was_five_evals[i];
    return rc;
  };
  for (int i = 0; i < count; i++) {
    agbnp_hip_context* const c = ctxs[i];
    was_enqueued[i] = c->enqueued;
    was_five_evals[i] = c->five_evals;
    single.lift(c, reqs[i]);
    const int rc = enqueue_prepare(c, reqs[i], plans[i]);
    prepared = i + 1;
    if (rc != AGBNP_HIP_OK) return undo(rc);
    shares[i] = group_shares(c, plans[i], reqs[i]);
    done[i] = !shares[i];
  }
  for (int i = 0; i < count; i++) {
    if (done[i]) continue;
    const agbnp_hip_context* a = ctxs[i];
    int set[kMaxGroup], m = 0;
    for (int j = i; j < count; j++) {
      const agbnp_hip_context* b = ctxs[j];
      if (!done[j] && b->version == a->version && b->variant == a->variant && b->P.gb_far == a->P.gb_far) set[m++] = j, done[j] = true;
    }
    for (int k = 0; k < m; k++) launched[set[k]] = true;
    // (a launch set of one makes the member's own launches: the same kernels without the look-up of its argument block, which
    // costs a dependent scalar load in front of every launch's first use of an argument)
    const int rc = m > 1 ? launch_set(ctxs, set, m, plans, reqs) : enqueue_launch(ctxs[set[0]], plans[set[0]], reqs[set[0]]);
    if (rc != AGBNP_HIP_OK) return undo(rc);
    if (m == 1) ctxs[set[0]]->group_members = 1;
  }
  for (int i = 0; i < count; i++) {
    if (shares[i]) continue;
    launched[i] = true;
    const int rc = enqueue_launch(ctxs[i], plans[i], reqs[i]);
    if (rc != AGBNP_HIP_OK) return undo(rc);
  }
  return AGBNP_HIP_OK;
}

// The device forms.  agbnp_hip_execute_group; agbnp_hip_energy_group: for every member what agbnp_hip_energy_device would do, the
// sharing members on FOUR (version 0: two) launches per launch set, nothing written to a force buffer of a caller;
// agbnp_hip_decompose_group: for every member what agbnp_hip_decompose_device would do (d_energies may be null), the sharing
// members on FIVE (version 0: three) launches per launch set; agbnp_hip_pair_matrix_group: for every member what
// agbnp_hip_pair_matrix_device would do, on as many launches
int group_device(agbnp_hip_context* const* ctxs, int count, const GroupCall& g, void* stream) {
  int rc = check_group(ctxs, count, g);
  if (rc != AGBNP_HIP_OK) return rc;
  agbnp_hip_context* const c0 = ctxs[0];
  hipStream_t st;
  rc = enter(c0, stream, &st);
  if (rc != AGBNP_HIP_OK) return rc;
  const bool full = g.kind == GroupKind::full, decomposition = g.kind == GroupKind::decomposition, matrix = g.kind == GroupKind::matrix;
  const Analysis analysis = analysis_of(g.kind);
  if (is_capturing(st))
    return c0->fail(AGBNP_HIP_ERR_INVALID_ARGUMENT,
                    std::string(g.who) + ": the stream is being captured; " +
                        (g.kind == GroupKind::perturb ? "groups and perturbation energies" : matrix ? "groups and pair matrices" : decomposition ? "groups and decompositions" : full ? "groups" : "groups and energy-only evaluations") +
                        " are not captured into graphs");
  EvalRequest reqs[kMaxGroup];
  for (int i = 0; i < count; i++) {
    agbnp_hip_context* const c = ctxs[i];
    HIP_TRY(c, hipSetDevice(c->device));
    // (NULL: the first member's own stream, which no caller can name -- it is not noted as a caller stream; every member's own
    // stream is joined to it on both sides instead, so that the member's agbnp_hip_finish(NULL) drains the group's work)
    note_stream(c, stream);
    if (!stream) HIP_TRY(c, join_streams(c->group_event, c->stream, st));
    if (!full) {  // (an analysis without energy words: into the member's spare word, as agbnp_hip_decompose_device)
      reqs[i] = energy_request(c, g.pos[i], g.d_energies ? g.d_energies[i] : nullptr, st, analysis, analysis != Analysis::none ? g.planes[i] : nullptr);
      continue;
    }
    reqs[i].pos = g.pos[i];
    reqs[i].force = g.forces[i];
    reqs[i].energy = g.d_energies[i];
    reqs[i].stream = st;
  }
  rc = group_enqueue(ctxs, count, reqs);
  if (rc != AGBNP_HIP_OK) return rc;
  for (int i = 0; i < count && !stream; i++) HIP_TRY(ctxs[i], join_streams(ctxs[i]->group_event, st, ctxs[i]->stream));
  return AGBNP_HIP_OK;
}

// The host forms' per-kind steps.  A member stages in d_force_tmp [3n + 1] -- forces and energy in one buffer, cleared by the cavity
// launch's trailing workgroups as in agbnp_hip_execute_host -- or, an analysis, in d_decomp [4n + 1] or [S S + 1] (stage_analysis) ...
int stage_member(agbnp_hip_context* c, const GroupCall& g, int i, hipStream_t st, EvalRequest* r) {
  if (is_analysis(g.kind))
    return stage_analysis(c, g.pos[i], analysis_of(g.kind), target_words(c, g.kind), st, r);
  HIP_TRY(c, hipMemcpyAsync(c->d_pos_in.p, g.pos[i], sizeof(double) * 3 * (size_t)c->n, hipMemcpyHostToDevice, st));
  r->pos = c->d_pos_in.p;
  r->force = g.kind == GroupKind::full ? c->d_force_tmp.p : c->d_eo_force.p;
  r->energy = c->d_force_tmp.p + 3 * (size_t)c->n;
  r->stream = st;
  r->energy_only = g.kind != GroupKind::full;
  r->zero_out = c->d_force_tmp.p;
  return AGBNP_HIP_OK;
}
// ... a member whose evaluation was withheld is repeated alone, as its own host entry point repeats ...
int repeat_member(agbnp_hip_context* c, const GroupCall& g, int i) {
  if (g.kind == GroupKind::decomposition) return host_decomposition(c, g.pos[i], g.planes[i], &g.energies[i]);
  if (g.kind == GroupKind::matrix) return agbnp_hip_pair_matrix_host(c, g.pos[i], g.planes[i], &g.energies[i]);
  if (g.kind == GroupKind::perturb) return agbnp_hip_perturbed_energies_host(c, g.pos[i], g.planes[i], &g.energies[i]);
  return host_evaluation(c, g.pos[i], g.kind == GroupKind::full ? g.forces[i] : nullptr, &g.energies[i]);
}
// ... and what came back is delivered once the stream is idle: forces ADDED and the energy stored, the energy alone, or the planes
// or the matrix OVERWRITTEN (read back in front of the harvest: fetch_analysis; the other two with blocking copies here)
int deliver_member(agbnp_hip_context* c, const GroupCall& g, int i, const EvalRequest& r) {
  const size_t n3 = 3 * (size_t)c->n;
  if (is_analysis(g.kind)) deliver_analysis(c, target_words(c, g.kind), g.planes[i], &g.energies[i]);
  if (g.kind == GroupKind::energy_only) HIP_TRY(c, hipMemcpy(&g.energies[i], r.energy, sizeof(double), hipMemcpyDeviceToHost));
  if (g.kind != GroupKind::full) return AGBNP_HIP_OK;
  c->h_force_tmp.resize(n3 + 1);
  HIP_TRY(c, hipMemcpy(c->h_force_tmp.data(), c->d_force_tmp.p, sizeof(double) * (n3 + 1), hipMemcpyDeviceToHost));
  for (size_t k = 0; k < n3; k++) g.forces[i][k] += c->h_force_tmp[k];
  g.energies[i] = c->h_force_tmp[n3];
  return AGBNP_HIP_OK;
}

// agbnp_hip_execute_group_host, agbnp_hip_energy_group_host, agbnp_hip_decompose_group_host, agbnp_hip_pair_matrix_group_host: one
// skeleton over the kind
int group_host(agbnp_hip_context* const* ctxs, int count, const GroupCall& g) {
  int rc = check_group(ctxs, count, g);
  if (rc != AGBNP_HIP_OK) return rc;
  const hipStream_t st = ctxs[0]->stream;
  EvalRequest reqs[kMaxGroup];
  for (int i = 0; i < count; i++) {
    agbnp_hip_context* const c = ctxs[i];
    HIP_TRY(c, hipSetDevice(c->device));
    rc = carry_unfinished(c);  // (every member's streams are idle from here on)
    if (rc == AGBNP_HIP_OK) rc = stage_member(c, g, i, st, &reqs[i]);
    if (rc != AGBNP_HIP_OK) return rc;
  }
  rc = group_enqueue(ctxs, count, reqs);
  if (rc != AGBNP_HIP_OK) return rc;
  for (int i = 0; i < count; i++) {
    agbnp_hip_context* const c = ctxs[i];
    if (is_analysis(g.kind)) HIP_TRY(c, fetch_analysis(c, target_words(c, g.kind), st));
    int repeat = 0;
    rc = harvest(c, &repeat, st);  // (waits for the group's stream)
    if (rc == AGBNP_HIP_OK) rc = repeat ? repeat_member(c, g, i) : deliver_member(c, g, i, reqs[i]);
    if (rc != AGBNP_HIP_OK) return rc;
  }
  return AGBNP_HIP_OK;
}
}  // namespace

extern "C" {

int agbnp_hip_decompose_group(agbnp_hip_context* const* ctxs, int count, const double* const* d_positions, double* const* d_per_atom,
                              double* const* d_energies, void* stream) {
  return group_device(ctxs, count, {GroupKind::decomposition, "agbnp_hip_decompose_group", false, d_positions, nullptr, d_per_atom, d_energies, nullptr}, stream);
}

int agbnp_hip_decompose_group_host(agbnp_hip_context* const* ctxs, int count, const double* const* positions, double* const* per_atom,
                                   double* energies) {
  return group_host(ctxs, count, {GroupKind::decomposition, "agbnp_hip_decompose_group_host", true, positions, nullptr, per_atom, nullptr, energies});
}

int agbnp_hip_pair_matrix_group(agbnp_hip_context* const* ctxs, int count, const double* const* d_positions, double* const* d_matrices,
                                double* const* d_energies, void* stream) {
  return group_device(ctxs, count, {GroupKind::matrix, "agbnp_hip_pair_matrix_group", false, d_positions, nullptr, d_matrices, d_energies, nullptr}, stream);
}

int agbnp_hip_pair_matrix_group_host(agbnp_hip_context* const* ctxs, int count, const double* const* positions, double* const* matrices,
                                     double* energies) {
  return group_host(ctxs, count, {GroupKind::matrix, "agbnp_hip_pair_matrix_group_host", true, positions, nullptr, matrices, nullptr, energies});
}

int agbnp_hip_perturbed_energies_group(agbnp_hip_context* const* ctxs, int count, const double* const* d_positions,
                                       double* const* d_energies, double* const* d_own_energies, void* stream) {
  return group_device(ctxs, count, {GroupKind::perturb, "agbnp_hip_perturbed_energies_group", false, d_positions, nullptr, d_energies, d_own_energies, nullptr}, stream);
}

int agbnp_hip_perturbed_energies_group_host(agbnp_hip_context* const* ctxs, int count, const double* const* positions,
                                            double* const* energies, double* own_energies) {
  return group_host(ctxs, count, {GroupKind::perturb, "agbnp_hip_perturbed_energies_group_host", true, positions, nullptr, energies, nullptr, own_energies});
}

int agbnp_hip_execute_group(agbnp_hip_context* const* ctxs, int count, const double* const* d_positions, double* const* d_forces,
                            double* const* d_energies, void* stream) {
  return group_device(ctxs, count, {GroupKind::full, "agbnp_hip_execute_group", false, d_positions, d_forces, nullptr, d_energies, nullptr}, stream);
}

int agbnp_hip_execute_group_host(agbnp_hip_context* const* ctxs, int count, const double* const* positions, double* const* forces,
                                 double* energies) {
  return group_host(ctxs, count, {GroupKind::full, "agbnp_hip_execute_group_host", true, positions, forces, nullptr, nullptr, energies});
}

int agbnp_hip_energy_group(agbnp_hip_context* const* ctxs, int count, const double* const* d_positions, double* const* d_energies,
                           void* stream) {
  return group_device(ctxs, count, {GroupKind::energy_only, "agbnp_hip_energy_group", false, d_positions, nullptr, nullptr, d_energies, nullptr}, stream);
}

int agbnp_hip_energy_group_host(agbnp_hip_context* const* ctxs, int count, const double* const* positions, double* energies) {
  return group_host(ctxs, count, {GroupKind::energy_only, "agbnp_hip_energy_group_host", true, positions, nullptr, nullptr, nullptr, energies});
}

}  // extern "C"
