// One evaluation of one context (engine_context.h): the request and how it enters and leaves the argument blocks, the
// per-evaluation host logic and the launches -- the analysis that a request carries among them --, the harvest behind them, and
// every single-context entry point that computes.
#include "engine_context.h"

// set the context's device and pick the stream of a call: the caller's, or the context's own
int enter(agbnp_hip_context* c, void* stream, hipStream_t* st) {
  HIP_TRY(c, hipSetDevice(c->device));
  *st = stream ? (hipStream_t)stream : c->stream;
  return AGBNP_HIP_OK;
}

// reads of the device that agbnp_hip_execute_host's short cut has put off (its stream is idle: every call ends with a wait);
// in front of every diagnostic read
int catch_up(agbnp_hip_context* c) {
  if (c->lazy_evals == 0) return AGBNP_HIP_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  int none = 0;
  return harvest(c, &none, c->stream);  // (every one of them was complete: nothing to repeat)
}

void note_stream(agbnp_hip_context* c, void* stream) {  // a caller's stream with work of this context on it
  c->unfinished = true;
  if (stream && std::find(c->user_streams.begin(), c->user_streams.end(), stream) == c->user_streams.end()) c->user_streams.push_back(stream);
}

// Energy-only evaluations (agbnp_hip_energy_*) run on launches of their own where the context runs the five-launch mode with the
// host-named set, the Reference semantics and -- version 1 -- the FP64 row form of the pair stages: the cavity launch, then
// launch_energy_only_stages (no chain-rule launch, no pseudo-volume launch).  Everywhere else (deterministic, fast, fast+single
// modes, AGBNP_HIP_ROWS=0, AGBNP_HIP_FIVE_LAUNCHES=0, capacity variant 4, diagnostics, a context captured into a graph before)
// they run as full evaluations whose forces go to a buffer of the context's own.
bool energy_only_fast(const agbnp_hip_context* c) {
  if (!c->five_active || c->five_device || c->mode != 0 || c->variant > 3 || c->diagnostics || c->nh <= 0) return false;
  if (c->version == 0) return true;
  return c->P.rows_on && !c->P.gb_rows && !c->P.single && !c->P.fast && !c->P.det;
}

// The words beside the work-slot rows change their meaning (or their contents, host upload or launch, for the other entry point): a
// graph captured through the entry point of the old kind has frozen the cavity kernel that reads them the old way -- its next
// replay would take slots for atom indices or the reverse, both below n, nothing faults -- so it is stale, and the generation
// says so.  Also when the change is enqueued inside a stream capture (k_row_atoms then replays with that graph, which stays
// right; the caller reads the generation after the capture): a graph captured EARLIER through the other entry point is stale
// from that graph's first replay on.  Host bookkeeping only: no launch, nothing in a steady run.
void set_row_atoms_kind(agbnp_hip_context* c, int kind) {
  if (c->row_atoms_kind == kind) return;
  c->row_atoms_kind = kind;
  c->generation++;
}

bool is_capturing(hipStream_t st) {
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  return hipStreamIsCapturing(st, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone;
}

namespace {
// The one place a request enters the argument blocks (the kernel arguments are captured by value at launch, so it is there for this
// evaluation only).  Five-launch mode: the tree reads the caller's positions itself ...
void bind_request(agbnp_hip_context* c, const EvalRequest& r) {
  c->P.pos = r.pos;
  c->P.zero_out = r.zero_out;  // (cleared by k_prep / the cavity launch's trailing workgroups)
  // (member by member: launch_set compares a member's block bytewise, and a copy of the whole struct may bring the padding of a
  // request that lives on a caller's stack along -- the blocks' own padding stays zero)
  OpenmmSource& in = c->P.in;
  in.posq = r.in.posq, in.correction = r.in.correction, in.is_double = r.in.is_double;
  in.atom_index = r.in.atom_index, in.hslot = r.in.hslot;
  OpenmmTargets& omm = c->P.omm;
  omm.force_fixed = r.omm.force_fixed, omm.padded = r.omm.padded, omm.ctx_slot = r.omm.ctx_slot;
  omm.energy_buffer = r.omm.energy_buffer, omm.energy_is_double = r.omm.energy_is_double, omm.energy_slot = r.omm.energy_slot;
  if (!c->five_active) return;
  c->T.pos = r.pos;
  // ... or an OpenMM context's posq (agbnp_hip_execute_openmm, round 6): the POSQ instantiation of the cavity launch reads it at
  // the context's slots
  c->T.posq = r.in.posq;
  c->T.posq_corr = r.in.correction;
  c->T.posq_double = r.in.is_double;
  c->T.hslot = r.in.hslot;
}
}  // namespace

// ... and the one place it leaves them (P.pos and the tree's copies are overwritten by the next request)
// (whole structs here, member by member in bind_request: a value-initialised temporary has zero padding, a caller's request need not)
Unbind::~Unbind() {
  for (int i = 0; i < count; i++) {
    ctxs[i]->P.zero_out = nullptr;
    ctxs[i]->P.in = OpenmmSource();
    ctxs[i]->P.omm = OpenmmTargets();
  }
}

// The per-evaluation host logic of an evaluation: scratch, the five-launch mode's exits, its set, the request, the one-off launches
// in front of the evaluation (the masks of a fresh context, the words beside the rows), the decision on the outputs.
int enqueue_prepare(agbnp_hip_context* c, const EvalRequest& r, EvalPlan& plan) {
  const hipStream_t st = r.stream;
  int rc = ensure_scratch(c);
  if (rc != AGBNP_HIP_OK) return rc;
  c->group_members = 0;
  c->enqueued++;
  c->P.tree_node_cap = tree_variant_node_cap(c->variant);  // the packing of the next evaluation is sized for the variant in use
  c->P.tree_atom_cap = tree_variant_atom_cap(c->variant);
  c->P.tree_slots = c->tree_slots[c->variant];
  Timeline* tl = c->timeline.enabled ? &c->timeline : nullptr;
  if (c->five_active) {
    // the mode ends for good where it cannot hold: the 32 768-node store in HBM (variant 4), pair stages other than the FP64 row form (the renewal of the neighbour masks rides in the Born rows' launch), the
    // diagnostic pass-1 self volumes (a kernel instantiation of the six-launch path only).  (A stream capture is fine: the
    // evaluation's parity lives on the device.)
    // Version 0 (round 6: TWO launches -- the cavity launch with its trailing workgroups, the output launch, whose tail carries the
    // masks' renewal) takes the host-named set only: its bookkeeping role, which advances the device's evaluation counter, runs
    // INSIDE the output launch beside the workgroups that would have to read the counter, so a stream capture ends the mode there.
    // (Round 6 too: pair stages other than the FP64 row form -- the tile kernels of the deterministic mode and of AGBNP_HIP_ROWS=0, the
    // single-precision rows of the fast mode -- stay in the mode with the host-named set: the masks' renewal rides at the tail of
    // the GB tile launch / of the single-precision Born rows; a stream capture ends the mode for them as well.)
    const bool host_set_only = c->version == 0 || !c->P.rows_on || c->P.single;
    const bool capturing = host_set_only && !c->five_device && is_capturing(st);
    if (c->variant > 3 || c->nh <= 0 || c->diagnostics || capturing || (host_set_only && c->five_device)) {
      c->five_active = false;
      c->parity = 0;
      apply_parity(c);
      c->generation++;
    }
  }
  bind_request(c, r);
  // workgroups of the tree launches: what the device keeps resident for this variant (they take forests from a queue);
  // fewer if there cannot be that many forests
  plan.tree_grid = std::max(1, std::min(c->slot_cap, c->tree_slots[c->variant]));
  if (c->five_active) {
    if (!c->five_device && is_capturing(st)) {
      // a replayed graph freezes its kernel arguments: from here on the kernels take the evaluation's set from the device's own
      // count (which has kept step with the host's so far), for good -- the host cannot count replays
      c->five_device = true;
      c->generation++;
    }
    apply_parity(c);
    c->five_evals++;
    c->T.out.h2a = c->P.h2a;  // (the forest workgroups find a candidate's atom through it)
    // an OpenMM context's posq: the words beside the rows must then hold SLOTS -- the dealing role writes them for the entry point of
    // the evaluation it runs in, so they are rewritten here when this evaluation comes through the other one, or when the
    // context's order has changed since (one small launch, never in a steady run)
    const int want_kind = r.in.posq ? 1 : 0;
    if (c->row_atoms_kind != want_kind) {
      HIP_TRY(c, launch_row_atoms(c->slot_cap, c->d_rows.p, want_kind ? c->d_hslot.p : c->P.h2a, c->d_row_atoms.p, st));
      set_row_atoms_kind(c, want_kind);
    }
    // (agbnp_hip_expect_jump; inside a stream capture it stays pending: a captured mask launch would repeat at every replay)
    const bool jump = c->jump_expected && !is_capturing(st);
    if (!c->masks_valid || jump) {  // a fresh context, an OpenMM context that has reordered its atoms (harvest), a jump the caller has announced: lay them down anew
      HIP_TRY(c, launch_masks(c->P, st, tl));
      c->masks_valid = true;
      if (jump) c->jump_expected = false;
    }
  }
  if (!c->five_active) c->jump_expected = false;  // (the k_prep path lays the masks down at every evaluation)
  if (c->version == 1) {
    // The forces leave with the pseudo-volume launch when that launch is one round of workgroups (1dwc: -1 us, A/B on one
    // box).  With more forests than resident workgroups a workgroup replays several forests in a row, and the next
    // forest's loads queue behind the force atomics of the one before (three adds on one line of the caller's [n][3]
    // buffer retire more slowly than the heavy-atom table's separate rows: lattice of 16.6 k atoms 49 -> 99 us): there the
    // output launch stays.  (No heavy atom: no tree launch to carry them.)
    // (Round 4: the replay of queued forests is pipelined -- the next forest's data are asked for in front of the flush -- and
    // the forces were tried in the launch again: lattice k_tree_pseudo 51 -> 109 us once more.  On gfx9 loads, stores and
    // atomics share one in-order counter, and a wait that crosses the loop's back edge is a wait for everything, the
    // flush's atomics included.)
    // (Round 5: a system with more subtrees than that whose forests nevertheless fit ONE round -- 2clr under the rounds rule of
    // the packing: 3084 subtrees in 1280 forests -- is told by the forest count of the last evaluation the host has seen;
    // a stale hint costs time, never correctness.)
    const bool one_round = c->forests_hint > 0 && c->forests_hint <= c->tree_slots[c->variant];
    plan.fused = c->nh > 0 && (c->nh <= 2 * c->tree_slots[c->variant] || one_round);
  }
  return AGBNP_HIP_OK;
}

// the outputs of the pseudo-volume launch (TreeOutputs, tree_kernels.h)
void set_outputs(agbnp_hip_context* c, double* d_force, bool fused) {
  TreeOutputs& O = c->T.out;
  O.enabled = fused ? 1 : 0;
  O.n = c->n;
  O.a2h = c->P.a2h;
  O.h2a = c->P.h2a;
  O.force = c->P.omm.force_fixed ? nullptr : d_force;
  O.force_fixed = c->P.omm.force_fixed;
  O.padded = c->P.omm.padded;
  O.ctx_slot = c->P.omm.ctx_slot;
  O.gb_f = c->P.gb_fx;
  O.db_f = c->P.db_fx;
  O.rows_on = c->P.rows_on;
  O.bw = c->P.bw;
  O.grec = c->P.grec;
  O.hrec = c->P.hrec;
  O.nl_flag = c->P.nl_flag;
  O.nl_nitems = c->P.nl_nitems;
  O.row_target = c->P.row_target;
  O.gb_rows = c->P.gb_rows;
}

// The launches of an evaluation that enqueue_prepare has prepared, and behind them -- on every way out -- the request's analysis
int enqueue_launch(agbnp_hip_context* c, const EvalPlan& plan, const EvalRequest& r) {
  const hipStream_t st = r.stream;
  Timeline* tl = c->timeline.enabled ? &c->timeline : nullptr;
  const int tree_grid = plan.tree_grid;
  const PairLaunchShape shape = pair_launch_shape(c->P, c->version);
  const bool matrix = r.analysis == Analysis::matrix, perturb = r.analysis == Analysis::perturb;
  c->last_kind = perturb ? 5 : matrix ? 4 : r.sv_large() ? 3 : !r.energy_only ? 0 : (energy_only_fast(c) ? 1 : 2);
  // the form of the cavity launch and, with it, the replay's weights (tree_single_gather; the self volumes of pass 1 -- an
  // analysis, the diagnostics -- come out of that pass's own gather: both gathers there)
  c->T.single_gather = tree_single_gather(c->variant, c->version) && !r.sv_large() && !c->T.want_sv_large ? 1 : 0;
  auto analysis = [&]() -> int {
    if (!r.sv_large()) return AGBNP_HIP_OK;
    const hipError_t e = perturb  ? launch_perturb(c->P, c->psets, c->version, r.target, st)
                         : matrix ? launch_pair_matrix(c->P, c->sets, c->version, r.target, st, tl)
                                  : launch_decompose(c->P, c->version, r.target, st, tl);
    return e == hipSuccess ? AGBNP_HIP_OK : c->hipfail(e, perturb ? "launch_perturb" : matrix ? "launch_pair_matrix" : "launch_decompose");
  };
  if (c->five_active) {
    if (tl) HIP_TRY(c, tl->mark(kKTreeCavity, st));
    HIP_TRY(c, launch_tree_cavity_five(c->variant, tree_grid, c->T, c->P, st, r.sv_large()));
    if (r.energy_only && energy_only_fast(c)) {
      HIP_TRY(c, launch_energy_only_stages(c->P, shape, c->version, r.energy, c->d_components.p, st, tl));
      return analysis();
    }
  } else {
    HIP_TRY(c, launch_prep(c->P, st, tl));
    if (tl) HIP_TRY(c, tl->mark(kKTreeCavity, st));
    HIP_TRY(c, launch_tree_cavity(c->variant, kGlobalGrid, tree_grid, c->T, st, r.sv_large()));
  }
  if (c->version == 1) {
    HIP_TRY(c, launch_pair_stages(c->P, shape, r.energy, c->d_components.p, st, tl));
    if (tl) HIP_TRY(c, tl->mark(kKTreePseudo, st));
    // the forces leave with the pseudo-volume launch itself (TreeOutputs, tree_kernels.h): no output launch (enqueue_prepare)
    const bool fused = plan.fused;
    set_outputs(c, r.force, fused);
    HIP_TRY(c, launch_tree_pseudo(c->variant, kGlobalGrid, tree_grid, c->T, st));
    if (fused) {
      if (tl) HIP_TRY(c, tl->mark(-1, st));
      return analysis();
    }
  }
  // (version 0 in the five-launch mode: the renewal of the level-2 neighbour masks rides at the tail of this launch)
  HIP_TRY(c, launch_outputs(c->P, c->five_active && c->version == 0 ? shape.out_masks : shape.out, c->version, r.force, r.energy, c->d_components.p, st, tl));
  return analysis();
}

namespace {
int enqueue(agbnp_hip_context* c, const EvalRequest& r) {
  LiftSingle single;  // (in front of the Unbind: the option comes back behind it)
  const Unbind unbind{&c, 1};
  single.lift(c, r);
  EvalPlan plan;
  const int rc = enqueue_prepare(c, r, plan);
  if (rc != AGBNP_HIP_OK) return rc;
  return enqueue_launch(c, plan, r);
}
}  // namespace

// after the stream is idle: read status + components; react to overflow.  *repeat = number of evaluations since the
// previous harvest whose forces and energy were withheld on the device (the caller must run those again).
int harvest(agbnp_hip_context* c, int* repeat, hipStream_t st) {
  *repeat = 0;
  // what is read of the device: asked for behind everything on the stream, then ONE wait (the report: in pinned memory, or
  // -- without the pinned staging -- in the context)
  agbnp_hip_context::HostReport* r = c->h_report ? c->h_report : &c->own_report;
  HIP_TRY(c, hipMemcpyAsync(r->status, c->d_status.p, sizeof(r->status), hipMemcpyDeviceToHost, st));
  if (c->five_active) {  // (the words of ONE evaluation live in its parity's block: both blocks come along, the counter says which)
    HIP_TRY(c, hipMemcpyAsync(r->five, c->d_estatus.p, sizeof(r->five), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(&r->epoch, c->P.epoch_tree, sizeof(int), hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(c, hipMemcpyAsync(r->components, c->d_components.p, sizeof(r->components), hipMemcpyDeviceToHost, st));
  if (c->rows_capable) HIP_TRY(c, hipMemcpyAsync(r->rows, c->d_nl_flag.p, sizeof(r->rows), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(r->pack, c->d_forest.p + c->slot_cap + kPackState, sizeof(r->pack), hipMemcpyDeviceToHost, st));
  // ... and a new log starts behind the reads, in front of the same wait (an empty log is cleared to what it is)
  HIP_TRY(c, hipMemsetAsync(c->d_status.p + kStatEvalSeq, 0, sizeof(int) * (kStatTotalWords - kStatEvalSeq), st));
  HIP_TRY(c, hipStreamSynchronize(st));
  // per-kernel durations of everything enqueued since the last harvest
  Timeline& tl = c->timeline;
  for (size_t k = 0; k + 1 < tl.used; k++) {
    const int id = tl.ids[k];
    if (id < 0) continue;
    float ms = 0.f;
    HIP_TRY(c, hipEventElapsedTime(&ms, tl.events[k], tl.events[k + 1]));
    c->kernel_ms[id] += ms;
    c->kernel_launches[id]++;
  }
  tl.used = 0;
  std::memcpy(c->last_status, r->status, sizeof(r->status));
  if (c->five_active) {
    // (device count: the last evaluation took epoch & 1 BEFORE its bookkeeping role advanced the counter; the host's count is one ahead as well)
    c->parity = c->five_device ? (r->epoch + 1) & 1 : (c->five_evals + 1) & 1;
    std::memcpy(c->last_status, r->five + kStatBlockStride * c->parity, sizeof(int) * kStatEvalWords);
  }
  std::memcpy(c->last_components, r->components, sizeof(r->components));
  if (c->rows_capable) std::memcpy(c->last_rows, r->rows, sizeof(r->rows));
  std::memcpy(c->last_pack, r->pack, sizeof(r->pack));
  const int* s = c->last_status;
  c->withheld.clear();
  c->withheld_count = s[kStatBadCount];
  if (s[kStatEvalSeq] > 0) c->forests_hint = s[kStatForests];  // (what the NEXT evaluation runs on, written by the last one's bookkeeping)
  // the last evaluation's own words say whether the diagnostics on the device are those of a complete evaluation
  c->have_results = s[kStatEvalSeq] > 0 ? !(s[kStatNodeOverflow] | s[kStatAtomOverflow] | s[kStatPackOverflow] | s[kStatOrderStale] | s[kStatRowOverflow]) : c->have_results;
  if (c->h_status) c->h_status[0] = c->h_status[1] = 0;  // (the stream is idle: nothing writes it now)
  const int host_first = c->lazy_evals;  // the log's first entries are execute_host's own (every one of them complete)
  c->last_device_seq = std::max(0, s[kStatEvalSeq] - host_first);
  c->enqueued = 0;  // (the device's running number starts over with the log)
  c->lazy_evals = 0;
  if (c->withheld_count == 0) return AGBNP_HIP_OK;
  for (int k = host_first; k < kStatBadBits && k < s[kStatEvalSeq]; k++)
    if (s[kStatBadBitmap + (k >> 5)] & (1 << (k & 31))) c->withheld.push_back(k - host_first);
  *repeat = c->withheld_count;
  // A repeat must not overflow for the same reason again: it runs one work item per work slot (the packing of the
  // evaluation that follows a withheld one is otherwise planned from whatever evaluation ran last), and if a lone item
  // outgrew the store while its subtree was shared by fewer than four, every subtree is shared four ways from here on
  // (straight to four: one repeat instead of a ladder of them; the fallback only ever runs repeats) ...
  // It stays at four when the capacity variant is raised below (ADVICE r04 asked for a reset; measured: a geometry that has to
  // climb several variants -- test_graph_replay_..., 5527-node subtree -- then pays TWO repeats per variant, whole subtrees
  // first and four-way next, instead of one; the fallback only ever runs repeats, the planned packings decide the parts from
  // the measured shapes whatever this says)
  const bool raise = s[kStatStickyNode] || s[kStatStickyAtom];
  if (s[kStatStickySplit] > 0) c->fallback_parts = 4;
  int rc = upload_identity_packing(c);
  if (rc != AGBNP_HIP_OK) return rc;
  c->forests_hint = 0;  // (one work item per slot again: the old rule decides)
  if (s[kStatStickyOrder] & 1) {
    c->order_valid = false;  // the context has reordered its atoms: the next agbnp_hip_execute_openmm rebuilds the maps
    // (five-launch mode: the device has renewed the neighbour masks in that evaluation -- from positions read through the STALE
    // maps, i.e. other atoms' positions: laid down anew by a launch of their own in front of the next evaluation)
    c->masks_valid = false;
  }
  // (bit 1, five-launch mode: a heavy atom had left the neighbour masks' skin.  The device has laid the masks down anew in
  // that very evaluation's Born launch: nothing for the host to do but repeat what was withheld)
  if (s[kStatStickyRow] && !c->rows_disabled) {
    // a neighbour list of the row-form pair stages outgrew what the launches walk of it: they walk twice as much from
    // here on -- or, if that already was the whole stride, the tile kernels take over (other launches either way: a
    // captured graph of this context is stale)
    const PairArgs& P = c->P;
    const bool whole = P.nlh_cap >= P.nlh_stride && P.nla_cap >= P.nla_stride && (!P.gb_rows || P.nlg_cap >= P.nlg_stride);
    if (whole) {
      c->rows_disabled = true;
    } else {
      c->row_boost *= 2;
      rc = mark_rows_stale(c);  // (the work items were laid down for the narrower walk: rebuilt with the lists)
      if (rc != AGBNP_HIP_OK) return rc;
    }
    derive_args(c);
    c->generation++;
  }
  if (raise) {
    // ... and, if a single subtree outgrew the store, on the next larger capacity variant
    if (c->variant >= kGlobalVariant)
      return c->fail(AGBNP_HIP_ERR_CAPACITY, "overlap subtree exceeds the largest supported capacity (32768 nodes / 255 partners per heavy atom)");
    c->variant++;
    c->generation++;  // other kernels, other scratch: a captured graph of this context is stale
  }
  // (a packed forest that outgrew its store: the device has already tightened its packing thresholds)
  return AGBNP_HIP_OK;
}

// The sticky overflow log is about to be read and cleared by a host-facing call's own harvest.  Evaluations that the caller
// has enqueued with agbnp_hip_execute_device and not yet finished must not lose their entries: they are harvested now and
// carried over to the caller's next agbnp_hip_finish.
int carry_unfinished(agbnp_hip_context* c) {
  if (!c->unfinished) return AGBNP_HIP_OK;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  for (void* st : c->user_streams) HIP_TRY(c, hipStreamSynchronize((hipStream_t)st));
  int pending = 0;
  int rc = harvest(c, &pending, c->stream);
  if (rc != AGBNP_HIP_OK) return rc;
  const int seq = c->last_device_seq;
  for (int k : c->withheld) c->carried.push_back(k + c->carried_seq);
  c->carried_count += pending;
  c->carried_seq += seq;
  c->unfinished = false;
  return AGBNP_HIP_OK;
}

// agbnp_hip_execute_host and agbnp_hip_energy_host: forces == nullptr is the energy-only evaluation (nothing but the energy
// travels back)
int host_evaluation(agbnp_hip_context* c, const double* pos, double* forces, double* energy) {
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t bytes = sizeof(double) * 3 * (size_t)c->n;
  int rc0 = carry_unfinished(c);
  if (rc0 != AGBNP_HIP_OK) return rc0;
  const size_t n3 = 3 * (size_t)c->n;
  EvalRequest r;
  r.pos = c->d_pos_in.p;
  r.force = r.zero_out = c->d_force_tmp.p;
  r.energy = c->d_force_tmp.p + n3;  // forces and energy leave in one buffer: one clear, one copy back
  r.stream = c->stream;
  r.energy_only = forces == nullptr;
  double* const h_in = c->h_xfer ? c->h_xfer : nullptr;
  double* const h_out = c->h_xfer ? c->h_xfer + n3 : c->h_force_tmp.data();
  if (h_in) std::memcpy(h_in, pos, bytes);
  for (int attempt = 0; attempt < 10; attempt++) {
    HIP_TRY(c, hipMemcpyAsync(c->d_pos_in.p, h_in ? h_in : pos, bytes, hipMemcpyHostToDevice, c->stream));
    int rc = enqueue(c, r);
    if (rc != AGBNP_HIP_OK) return rc;
    if (r.energy_only)
      HIP_TRY(c, hipMemcpyAsync(h_out + n3, r.energy, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    else
      HIP_TRY(c, hipMemcpyAsync(h_out, c->d_force_tmp.p, bytes + sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (c->h_status && c->h_report && !c->timeline.enabled && c->enqueued < 1024) {
      // the short cut: the device's own word on this evaluation (pinned memory, written when its tree stage had ended).
      // The wait for the stream is a spin on its status: a blocking wait comes back 10-20 us late.
      for (hipError_t q = hipStreamQuery(c->stream); q != hipSuccess; q = hipStreamQuery(c->stream))
        if (q != hipErrorNotReady) {
          HIP_TRY(c, q);
          break;
        }
      const volatile int* h = c->h_status;
      const int judged = h[0];
      std::atomic_thread_fence(std::memory_order_acquire);
      if (judged == c->enqueued && h[1] == 0) {
        c->lazy_evals++;
        for (size_t k = 0; k < n3 && forces; k++) forces[k] += h_out[k];
        *energy = h_out[n3];
        return AGBNP_HIP_OK;
      }
    }
    int repeat = 0;
    rc = harvest(c, &repeat, c->stream);  // (its own reads follow on the stream; one wait for everything)
    if (rc != AGBNP_HIP_OK) return rc;
    if (repeat) continue;
    for (size_t k = 0; k < n3 && forces; k++) forces[k] += h_out[k];
    *energy = h_out[n3];
    return AGBNP_HIP_OK;
  }
  return c->fail(AGBNP_HIP_ERR_CAPACITY, r.energy_only ? "agbnp_hip_energy_host: capacity negotiation did not converge"
                                                       : "agbnp_hip_execute_host: capacity negotiation did not converge");
}

namespace {
// the energy-only entry points launch nothing inside a stream capture (energy-only graphs are not supported)
bool refuse_capture(agbnp_hip_context* c, hipStream_t st, const char* who) {
  if (!is_capturing(st)) return false;
  c->fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, std::string(who) + ": the stream is being captured; energy-only evaluations cannot be captured into a graph (capture agbnp_hip_execute_device instead)");
  return true;
}

// the argument check of agbnp_hip_execute_openmm and agbnp_hip_energy_openmm; d_output: the buffer the call must be given
int check_openmm(agbnp_hip_context* c, const void* d_posq, int posq_is_double, const void* d_posq_correction, int padded_num_atoms,
                 const void* d_output, int energy_slot, const char* who) {
  if (!c) return AGBNP_HIP_ERR_INVALID_ARGUMENT;
  if (!d_posq || !d_output) return c->fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, std::string(who) + ": null pointer");
  if (padded_num_atoms < c->n) return c->fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, std::string(who) + ": padded atom count below the particle count");
  if (posq_is_double && d_posq_correction)
    return c->fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, std::string(who) + ": a position correction only exists beside float positions");
  if (energy_slot < 0) return c->fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, std::string(who) + ": negative energy slot");
  return AGBNP_HIP_OK;
}

// agbnp_hip_execute_openmm and agbnp_hip_energy_openmm (energy_only: d_force_buffer is the context's own), arguments checked
int agbnp_hip_execute_openmm_to(agbnp_hip_context* c, const void* d_posq, int posq_is_double, const void* d_posq_correction,
                                const int* d_atom_index, int padded_num_atoms, long long* d_force_buffer, void* d_energy_buffer,
                                int energy_is_double, int energy_slot, hipStream_t st, void* stream, bool energy_only) {
  note_stream(c, stream);
  EvalRequest r;
  r.pos = c->d_pos_in.p;
  r.force = c->d_force_tmp.p;
  r.energy = c->d_energy_tmp.p;
  r.stream = st;
  r.energy_only = energy_only;
  // Input side.  Normally k_prep reads the context's posq itself, through the engine's maps of the context's atom order
  // (OpenmmSource): they are built when an atomIndex array is first seen (or seen again after the device has found it
  // changed), one small launch that a steady run never repeats.  AGBNP_HIP_ADAPTER_LAUNCH=1: an adapter launch per
  // evaluation instead (posq -> xyz in particle order, and the particle -> slot map for the output side).
  const bool fused = !c->cfg.adapter_launch;
  if (fused) {
    if (!c->order_valid || c->order_ptr != d_atom_index) {
      HIP_TRY(c, launch_order_maps(c->n, d_atom_index, c->P.a2h, c->d_ctx_slot.p, c->d_hslot.p, st));
      if (c->row_atoms_kind == 1) set_row_atoms_kind(c, -1);  // (slots of the old order: enqueue rewrites them)
      c->order_valid = true;
      c->order_ptr = d_atom_index;
    }
    r.in.posq = d_posq;
    r.in.correction = static_cast<const float4*>(d_posq_correction);
    r.in.is_double = posq_is_double;
    r.in.atom_index = d_atom_index;
    r.in.hslot = c->d_hslot.p;
  } else {
    HIP_TRY(c, launch_adapt_positions(c->n, d_posq, posq_is_double, d_posq_correction, d_atom_index, c->d_pos_in.p, c->d_ctx_slot.p, st));
  }
  // the output side is the engine's own last kernel: forces as fixed point at the context's slots, energy into its
  // accumulator
  r.omm.force_fixed = reinterpret_cast<unsigned long long*>(d_force_buffer);
  r.omm.padded = padded_num_atoms;
  r.omm.ctx_slot = c->d_ctx_slot.p;
  r.omm.energy_buffer = d_energy_buffer;
  r.omm.energy_is_double = energy_is_double;
  r.omm.energy_slot = energy_slot;
  return enqueue(c, r);
}
}  // namespace

// The energy-only request -- the context's own force target, for where it runs as a full evaluation -- and with it the analysis that
// follows, if any (engine_context.h, above EvalRequest), set together.  d_energy null: the energy goes to the context's spare word.
EvalRequest energy_request(agbnp_hip_context* c, const double* d_pos, double* d_energy, hipStream_t st, Analysis kind, double* target) {
  EvalRequest r;
  r.pos = d_pos;
  r.force = c->d_eo_force.p;
  r.energy = d_energy ? d_energy : c->d_energy_tmp.p;
  r.stream = st;
  r.energy_only = true;
  r.analysis = kind;
  r.target = target;
  return r;
}

// A host form's analysis (agbnp_hip_decompose_host, agbnp_hip_pair_matrix_host, agbnp_hip_perturbed_energies_host, a member of a
// group's host form): the `count` words of the planes, of the matrix or of the energies under the sets, and the energy travel through one buffer [count + 1], cleared first (the device path
// ADDS).  stage_analysis: the buffers, the positions up, the clear, the request; fetch_analysis: the read-back, in front of the
// harvest's wait; deliver_analysis: what came back OVERWRITES the caller's
int stage_analysis(agbnp_hip_context* c, const double* pos, Analysis kind, size_t count, hipStream_t st, EvalRequest* r) {
  if (c->d_decomp.count != count + 1) HIP_TRY(c, c->d_decomp.alloc(count + 1));
  c->h_decomp.resize(count + 1);
  HIP_TRY(c, hipMemcpyAsync(c->d_pos_in.p, pos, sizeof(double) * 3 * (size_t)c->n, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemsetAsync(c->d_decomp.p, 0, sizeof(double) * (count + 1), st));
  *r = energy_request(c, c->d_pos_in.p, c->d_decomp.p + count, st, kind, c->d_decomp.p);
  return AGBNP_HIP_OK;
}
hipError_t fetch_analysis(agbnp_hip_context* c, size_t count, hipStream_t st) {
  return hipMemcpyAsync(c->h_decomp.data(), c->d_decomp.p, sizeof(double) * (count + 1), hipMemcpyDeviceToHost, st);
}
void deliver_analysis(const agbnp_hip_context* c, size_t count, double* out, double* energy) {
  std::memcpy(out, c->h_decomp.data(), sizeof(double) * count);
  *energy = c->h_decomp[count];
}

// agbnp_hip_decompose_host, agbnp_hip_pair_matrix_host, agbnp_hip_perturbed_energies_host: withheld evaluations are repeated
static int host_analysis(agbnp_hip_context* c, const double* pos, Analysis kind, size_t count, double* out, double* energy, const char* who) {
  HIP_TRY(c, hipSetDevice(c->device));
  const int rc0 = carry_unfinished(c);
  if (rc0 != AGBNP_HIP_OK) return rc0;
  for (int attempt = 0; attempt < 10; attempt++) {
    EvalRequest r;
    int rc = stage_analysis(c, pos, kind, count, c->stream, &r);
    if (rc == AGBNP_HIP_OK) rc = enqueue(c, r);
    if (rc != AGBNP_HIP_OK) return rc;
    HIP_TRY(c, fetch_analysis(c, count, c->stream));
    int repeat = 0;
    rc = harvest(c, &repeat, c->stream);  // (its own reads follow on the stream; one wait for everything)
    if (rc != AGBNP_HIP_OK) return rc;
    if (repeat) continue;
    deliver_analysis(c, count, out, energy);
    return AGBNP_HIP_OK;
  }
  return c->fail(AGBNP_HIP_ERR_CAPACITY, std::string(who) + ": capacity negotiation did not converge");
}

// (also how agbnp_hip_decompose_group_host repeats a member whose evaluation was withheld)
int host_decomposition(agbnp_hip_context* c, const double* pos, double* per_atom, double* energy) {
  return host_analysis(c, pos, Analysis::planes, 4 * (size_t)c->n, per_atom, energy, "agbnp_hip_decompose_host");
}

// agbnp_hip_energy_device (no analysis), agbnp_hip_decompose_device, agbnp_hip_pair_matrix_device,
// agbnp_hip_perturbed_energies_device, arguments checked (the kernel
// files' comments know this path by its earlier name, enqueue_decomposition)
static int device_energy(agbnp_hip_context* c, const double* d_pos, Analysis kind, double* target, double* d_energy, void* stream, const char* who) {
  hipStream_t st;
  const int rc = enter(c, stream, &st);
  if (rc != AGBNP_HIP_OK) return rc;
  if (refuse_capture(c, st, who)) return AGBNP_HIP_ERR_INVALID_ARGUMENT;
  note_stream(c, stream);
  return enqueue(c, energy_request(c, d_pos, d_energy, st, kind, target));
}

// the matrix calls need a partition (agbnp_hip_set_atom_sets)
static int need_sets(agbnp_hip_context* c, const char* who) {
  if (c->sets.num_sets > 0) return AGBNP_HIP_OK;
  return c->fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, std::string(who) + ": no partition has been set (agbnp_hip_set_atom_sets)");
}

// the perturbation calls need parameter sets (agbnp_hip_set_parameter_sets)
static int need_parameter_sets(agbnp_hip_context* c, const char* who) {
  if (c->psets.num_sets > 0) return AGBNP_HIP_OK;
  return c->fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, std::string(who) + ": no parameter sets have been set (agbnp_hip_set_parameter_sets)");
}

extern "C" {

int agbnp_hip_decompose_host(agbnp_hip_context* c, const double* pos, double* per_atom, double* energy) {
  if (!c) return AGBNP_HIP_ERR_INVALID_ARGUMENT;
  if (!pos || !per_atom || !energy) return c->fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, "agbnp_hip_decompose_host: null pointer");
  return host_decomposition(c, pos, per_atom, energy);
}

int agbnp_hip_decompose_device(agbnp_hip_context* c, const double* d_pos, double* d_per_atom, double* d_energy, void* stream) {
  if (!c) return AGBNP_HIP_ERR_INVALID_ARGUMENT;
  if (!d_pos || !d_per_atom) return c->fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, "agbnp_hip_decompose_device: null pointer");
  return device_energy(c, d_pos, Analysis::planes, d_per_atom, d_energy, stream, "agbnp_hip_decompose_device");
}

// The partition is the matrix launch's alone (AtomSets): nothing an evaluation reads changes, so neither does
// agbnp_hip_generation().  Its tables are replaced in place (their sizes depend on n alone), so matrix calls in flight are
// waited for first -- the context's own stream and the streams the caller has enqueued on, as agbnp_hip_update_parameters
// waits -- and nothing else is.  A refused partition leaves the one before it in place.
int agbnp_hip_set_atom_sets(agbnp_hip_context* c, int n, const int* set_of_atom, int num_sets) {
  if (!c) return AGBNP_HIP_ERR_INVALID_ARGUMENT;
  if (!set_of_atom) return c->fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, "agbnp_hip_set_atom_sets: null pointer");
  if (n != c->n) return c->fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, "agbnp_hip_set_atom_sets: the number of particles differs from the context's");
  if (num_sets < 1 || num_sets > AGBNP_HIP_MAX_SETS)
    return c->fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, "agbnp_hip_set_atom_sets: num_sets must be 1 .. AGBNP_HIP_MAX_SETS");
  for (int i = 0; i < n; i++)
    if (set_of_atom[i] < 0 || set_of_atom[i] >= num_sets)
      return c->fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, "agbnp_hip_set_atom_sets: atom " + std::to_string(i) + " names a set outside 0 .. num_sets - 1");
  std::vector<unsigned char> rank;
  std::vector<int> lists, counts;
  const int depth = atom_set_tables(n, set_of_atom, rank, lists, counts);
  HIP_TRY(c, hipSetDevice(c->device));
  if (c->sets.num_sets > 0) {  // (before the first partition no launch can be reading the tables)
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (void* st : c->user_streams) HIP_TRY(c, hipStreamSynchronize((hipStream_t)st));
  }
  c->sets = AtomSets{};  // (a failed upload leaves no partition rather than half of one)
  HIP_TRY(c, c->d_set_rank.upload(rank));
  HIP_TRY(c, c->d_set_lists.upload(lists));
  HIP_TRY(c, c->d_set_counts.upload(counts));
  c->sets.rank = c->d_set_rank.p;
  c->sets.block_sets = c->d_set_lists.p;
  c->sets.block_count = c->d_set_counts.p;
  c->sets.num_sets = num_sets;
  c->sets.depth = depth;
  return AGBNP_HIP_OK;
}

int agbnp_hip_num_atom_sets(const agbnp_hip_context* c) { return c ? c->sets.num_sets : 0; }

int agbnp_hip_pair_matrix_host(agbnp_hip_context* c, const double* pos, double* matrix, double* energy) {
  if (!c) return AGBNP_HIP_ERR_INVALID_ARGUMENT;
  if (!pos || !matrix || !energy) return c->fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, "agbnp_hip_pair_matrix_host: null pointer");
  const int rc = need_sets(c, "agbnp_hip_pair_matrix_host");
  if (rc != AGBNP_HIP_OK) return rc;
  const size_t S = (size_t)c->sets.num_sets;
  return host_analysis(c, pos, Analysis::matrix, S * S, matrix, energy, "agbnp_hip_pair_matrix_host");
}

int agbnp_hip_pair_matrix_device(agbnp_hip_context* c, const double* d_pos, double* d_matrix, double* d_energy, void* stream) {
  if (!c) return AGBNP_HIP_ERR_INVALID_ARGUMENT;
  if (!d_pos || !d_matrix) return c->fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, "agbnp_hip_pair_matrix_device: null pointer");
  const int rc = need_sets(c, "agbnp_hip_pair_matrix_device");
  if (rc != AGBNP_HIP_OK) return rc;
  return device_energy(c, d_pos, Analysis::matrix, d_matrix, d_energy, stream, "agbnp_hip_pair_matrix_device");
}

// The sets are the perturbation launch's alone (ParamSets), as the partition is the matrix launch's: nothing an evaluation reads
// changes, so neither does agbnp_hip_generation().  The tables are replaced (their sizes depend on M), so perturbation calls in
// flight are waited for first -- the context's own stream and the streams the caller has enqueued on -- and nothing else is.
// Refused sets leave the ones before them in place.
int agbnp_hip_set_parameter_sets(agbnp_hip_context* c, int n, int num_sets, const double* gamma, const double* vdw_alpha, const double* charge) {
  if (!c) return AGBNP_HIP_ERR_INVALID_ARGUMENT;
  if (!gamma || !vdw_alpha || !charge) return c->fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, "agbnp_hip_set_parameter_sets: null pointer");
  if (n != c->n) return c->fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, "agbnp_hip_set_parameter_sets: the number of particles differs from the context's");
  if (num_sets < 1 || num_sets > AGBNP_HIP_MAX_PARAMETER_SETS)
    return c->fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, "agbnp_hip_set_parameter_sets: num_sets must be 1 .. AGBNP_HIP_MAX_PARAMETER_SETS");
  const size_t words = (size_t)num_sets * (size_t)n;
  std::vector<double> nu(words);
  for (size_t k = 0; k < words; k++) nu[k] = c->ish[k % (size_t)n] ? 0.0 : gamma[k] / kRadiusIncrement;  // (as gam_cav: engine_setup.hip)
  HIP_TRY(c, hipSetDevice(c->device));
  if (c->d_pset_nu.p || c->d_pset_alpha.p || c->d_pset_charge.p) {  // (before the first tables no launch can be reading them; after a
                                                                    // failed upload they may stand without sets: still waited for)
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (void* st : c->user_streams) HIP_TRY(c, hipStreamSynchronize((hipStream_t)st));
  }
  c->psets = ParamSets{};  // (a failed upload leaves no sets rather than half of them)
  HIP_TRY(c, c->d_pset_nu.upload(nu));
  HIP_TRY(c, c->d_pset_alpha.upload(std::vector<double>(vdw_alpha, vdw_alpha + words)));
  HIP_TRY(c, c->d_pset_charge.upload(std::vector<double>(charge, charge + words)));
  c->psets.nu = c->d_pset_nu.p;
  c->psets.alpha = c->d_pset_alpha.p;
  c->psets.charge = c->d_pset_charge.p;
  c->psets.num_sets = num_sets;
  return AGBNP_HIP_OK;
}

int agbnp_hip_num_parameter_sets(const agbnp_hip_context* c) { return c ? c->psets.num_sets : 0; }

int agbnp_hip_perturbed_energies_host(agbnp_hip_context* c, const double* pos, double* energies, double* energy) {
  if (!c) return AGBNP_HIP_ERR_INVALID_ARGUMENT;
  if (!pos || !energies || !energy) return c->fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, "agbnp_hip_perturbed_energies_host: null pointer");
  const int rc = need_parameter_sets(c, "agbnp_hip_perturbed_energies_host");
  if (rc != AGBNP_HIP_OK) return rc;
  return host_analysis(c, pos, Analysis::perturb, (size_t)c->psets.num_sets, energies, energy, "agbnp_hip_perturbed_energies_host");
}

int agbnp_hip_perturbed_energies_device(agbnp_hip_context* c, const double* d_pos, double* d_energies, double* d_energy, void* stream) {
  if (!c) return AGBNP_HIP_ERR_INVALID_ARGUMENT;
  if (!d_pos || !d_energies) return c->fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, "agbnp_hip_perturbed_energies_device: null pointer");
  const int rc = need_parameter_sets(c, "agbnp_hip_perturbed_energies_device");
  if (rc != AGBNP_HIP_OK) return rc;
  return device_energy(c, d_pos, Analysis::perturb, d_energies, d_energy, stream, "agbnp_hip_perturbed_energies_device");
}

int agbnp_hip_execute_device(agbnp_hip_context* c, const double* d_pos, double* d_force, double* d_energy, void* stream) {
  if (!c) return AGBNP_HIP_ERR_INVALID_ARGUMENT;
  if (!d_pos || !d_force || !d_energy) return c->fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, "agbnp_hip_execute_device: null pointer");
  EvalRequest r;
  const int rc = enter(c, stream, &r.stream);
  if (rc != AGBNP_HIP_OK) return rc;
  note_stream(c, stream);
  r.pos = d_pos;
  r.force = d_force;
  r.energy = d_energy;
  return enqueue(c, r);
}

int agbnp_hip_energy_device(agbnp_hip_context* c, const double* d_pos, double* d_energy, void* stream) {
  if (!c) return AGBNP_HIP_ERR_INVALID_ARGUMENT;
  if (!d_pos || !d_energy) return c->fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, "agbnp_hip_energy_device: null pointer");
  return device_energy(c, d_pos, Analysis::none, nullptr, d_energy, stream, "agbnp_hip_energy_device");
}

int agbnp_hip_execute_openmm(agbnp_hip_context* c, const void* d_posq, int posq_is_double, const void* d_posq_correction,
                             const int* d_atom_index, int padded_num_atoms, long long* d_force_buffer, void* d_energy_buffer,
                             int energy_is_double, int energy_slot, void* stream) {
  int rc = check_openmm(c, d_posq, posq_is_double, d_posq_correction, padded_num_atoms, d_force_buffer, energy_slot, "agbnp_hip_execute_openmm");
  if (rc != AGBNP_HIP_OK) return rc;
  hipStream_t st;
  rc = enter(c, stream, &st);
  if (rc != AGBNP_HIP_OK) return rc;
  return agbnp_hip_execute_openmm_to(c, d_posq, posq_is_double, d_posq_correction, d_atom_index, padded_num_atoms, d_force_buffer,
                                     d_energy_buffer, energy_is_double, energy_slot, st, stream, false);
}

int agbnp_hip_energy_openmm(agbnp_hip_context* c, const void* d_posq, int posq_is_double, const void* d_posq_correction,
                            const int* d_atom_index, int padded_num_atoms, void* d_energy_buffer, int energy_is_double,
                            int energy_slot, void* stream) {
  int rc = check_openmm(c, d_posq, posq_is_double, d_posq_correction, padded_num_atoms, d_energy_buffer, energy_slot, "agbnp_hip_energy_openmm");
  if (rc != AGBNP_HIP_OK) return rc;
  hipStream_t st;
  rc = enter(c, stream, &st);
  if (rc != AGBNP_HIP_OK) return rc;
  if (refuse_capture(c, st, "agbnp_hip_energy_openmm")) return AGBNP_HIP_ERR_INVALID_ARGUMENT;
  const size_t planes = 3 * (size_t)padded_num_atoms;
  if (c->d_eo_fixed.count < planes)  // (hipFree of a smaller one waits for the device: nothing in flight still uses it)
    HIP_TRY(c, c->d_eo_fixed.alloc(planes, 0));
  // the same evaluation as agbnp_hip_execute_openmm, with the context's own fixed-point planes in place of the caller's
  return agbnp_hip_execute_openmm_to(c, d_posq, posq_is_double, d_posq_correction, d_atom_index, padded_num_atoms,
                                     reinterpret_cast<long long*>(c->d_eo_fixed.p), d_energy_buffer, energy_is_double, energy_slot, st, stream, true);
}

int agbnp_hip_execute_host(agbnp_hip_context* c, const double* pos, double* forces, double* energy) {
  if (!c) return AGBNP_HIP_ERR_INVALID_ARGUMENT;
  if (!pos || !forces || !energy) return c->fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, "agbnp_hip_execute_host: null pointer");
  return host_evaluation(c, pos, forces, energy);
}

int agbnp_hip_energy_host(agbnp_hip_context* c, const double* pos, double* energy) {
  if (!c) return AGBNP_HIP_ERR_INVALID_ARGUMENT;
  if (!pos || !energy) return c->fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, "agbnp_hip_energy_host: null pointer");
  return host_evaluation(c, pos, nullptr, energy);
}

int agbnp_hip_atom_order_changed(agbnp_hip_context* c) {
  if (!c) return AGBNP_HIP_ERR_INVALID_ARGUMENT;
  c->order_valid = false;
  return AGBNP_HIP_OK;
}

int agbnp_hip_expect_jump(agbnp_hip_context* c) {
  if (!c) return AGBNP_HIP_ERR_INVALID_ARGUMENT;
  if (c->five_active) c->jump_expected = true;  // (elsewhere k_prep lays the masks down at every evaluation: nothing to do)
  return AGBNP_HIP_OK;
}

int agbnp_hip_finish(agbnp_hip_context* c, void* stream, int* must_repeat) {
  if (!c) return AGBNP_HIP_ERR_INVALID_ARGUMENT;
  int dummy = 0;
  if (!must_repeat) must_repeat = &dummy;
  hipStream_t st;
  int rc = enter(c, stream, &st);
  if (rc != AGBNP_HIP_OK) return rc;
  c->user_streams.erase(std::remove(c->user_streams.begin(), c->user_streams.end(), stream), c->user_streams.end());
  rc = harvest(c, must_repeat, st);  // (waits for the stream)
  if (rc != AGBNP_HIP_OK) return rc;
  if (c->carried_count > 0) {
    // evaluations of execute_device that a call of agbnp_hip_execute_host in between had to harvest: they were enqueued
    // BEFORE everything this finish has just read, so they come first and the later indices move up
    for (int& k : c->withheld) k += c->carried_seq;
    c->withheld.insert(c->withheld.begin(), c->carried.begin(), c->carried.end());
    c->withheld_count += c->carried_count;
    *must_repeat = c->withheld_count;
  }
  c->carried.clear();
  c->carried_count = c->carried_seq = 0;
  c->unfinished = !c->user_streams.empty();
  return AGBNP_HIP_OK;
}

int agbnp_hip_poll(const agbnp_hip_context* c, int* evaluations_completed, int* withheld) {
  if (!c) return AGBNP_HIP_ERR_INVALID_ARGUMENT;
  if (!c->h_status) return AGBNP_HIP_ERR_DEVICE;
  const volatile int* h = c->h_status;
  const int done = h[0] - c->lazy_evals;  // (written after the withheld count, behind a system-scope fence; execute_host's own are not the caller's)
  std::atomic_thread_fence(std::memory_order_acquire);
  if (evaluations_completed) *evaluations_completed = done;
  if (withheld) *withheld = h[1];
  return AGBNP_HIP_OK;
}

int agbnp_hip_wait_verdict(const agbnp_hip_context* c, int evaluations, double timeout_seconds, int* evaluations_completed, int* withheld) {
  if (!c) return AGBNP_HIP_ERR_INVALID_ARGUMENT;
  if (!c->h_status) return AGBNP_HIP_ERR_DEVICE;
  const int target = evaluations > 0 ? evaluations + c->lazy_evals : c->enqueued;
  const volatile int* h = c->h_status;
  const auto t0 = std::chrono::steady_clock::now();
  int done = h[0];
  for (unsigned spins = 0; done < target; done = h[0]) {
    __builtin_ia32_pause();
    if ((++spins & 1023u) == 0 && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > timeout_seconds) break;
  }
  std::atomic_thread_fence(std::memory_order_acquire);  // (the withheld count is read AFTER the running number that vouches for it)
  if (evaluations_completed) *evaluations_completed = done - c->lazy_evals;
  if (withheld) *withheld = h[1];  // (written before the running number, behind a system-scope fence)
  return done >= target ? AGBNP_HIP_OK : AGBNP_HIP_ERR_TIMEOUT;
}

}  // extern "C"
