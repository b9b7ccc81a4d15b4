// What a caller reads back of a context (engine_context.h): the scalars and vectors of the last evaluation, the I4 tables, the
// per-kernel times, the small accessors -- and the diagnostic hooks of scripts/.
#include "engine_context.h"

extern "C" {

#ifndef AGBNP_SRC_HASH
#define AGBNP_SRC_HASH "unknown"  // (a build outside csrc/Makefile; scripts/build_diag.sh goes through it and marks its id with BUILD_TAG)
#endif
const char* agbnp_hip_build_id(void) { return AGBNP_SRC_HASH; }

int agbnp_hip_device_count(void) {
  int k = 0;
  if (hipGetDeviceCount(&k) != hipSuccess) return 0;
  return k;
}

const char* agbnp_hip_last_error(const agbnp_hip_context* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int agbnp_hip_get_scalar(agbnp_hip_context* c, int which, double* value) {
  if (!c || !value) return AGBNP_HIP_ERR_INVALID_ARGUMENT;
  const int rc_ = catch_up(c);
  if (rc_ != AGBNP_HIP_OK) return rc_;
  const int* s = c->last_status;
  switch (which) {  // what is valid whether or not an evaluation has completed
    case AGBNP_HIP_SCALAR_OVERFLOW_KINDS:
      *value = (s[kStatStickyNode] ? AGBNP_HIP_OVERFLOW_NODES : 0) | (s[kStatStickyAtom] ? AGBNP_HIP_OVERFLOW_ATOMS : 0) |
               (s[kStatStickyPack] ? AGBNP_HIP_OVERFLOW_PACKING : 0) | (s[kStatStickyRow] ? AGBNP_HIP_OVERFLOW_ROW : 0) |
               (s[kStatStickyOrder] ? AGBNP_HIP_OVERFLOW_REORDERED : 0) | (s[kStatStickyForest] * AGBNP_HIP_OVERFLOW_FOREST_NODES) |
               (s[kStatStickySplit] * AGBNP_HIP_OVERFLOW_SPLIT_PARTS);
      return AGBNP_HIP_OK;
    case AGBNP_HIP_SCALAR_ENERGY_ONLY_LAUNCHES: *value = energy_only_fast(c) ? (c->version == 1 ? 4 : 2) : 0; return AGBNP_HIP_OK;
    case AGBNP_HIP_SCALAR_GROUP_MEMBERS: *value = c->group_members; return AGBNP_HIP_OK;
    case AGBNP_HIP_SCALAR_LAST_EVALUATION_KIND: *value = c->last_kind; return AGBNP_HIP_OK;
    case AGBNP_HIP_SCALAR_GROUP_BLOCK_WRITES: *value = c->group_block_writes; return AGBNP_HIP_OK;
    case AGBNP_HIP_SCALAR_HEALED_FORESTS: *value = s[kStatStickyHealed]; return AGBNP_HIP_OK;
    default: break;
  }
  if (!c->have_results) return c->fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, "no completed evaluation yet");
  switch (which) {
    case AGBNP_HIP_SCALAR_E_VOL1: *value = c->last_components[0]; break;
    case AGBNP_HIP_SCALAR_E_VOL2: *value = c->last_components[1]; break;
    case AGBNP_HIP_SCALAR_E_ATOM: *value = c->last_components[2]; break;
    case AGBNP_HIP_SCALAR_E_GB_PAIR: *value = c->last_components[3]; break;
    case AGBNP_HIP_SCALAR_MAX_SUBTREE_NODES: *value = s[kStatMaxNodes]; break;
    case AGBNP_HIP_SCALAR_TOTAL_NODES: *value = s[kStatTotalNodes]; break;
    case AGBNP_HIP_SCALAR_VARIANT: *value = c->variant; break;
    case AGBNP_HIP_SCALAR_MAX_LOCAL_ATOMS: *value = s[kStatMaxAtoms]; break;
    case AGBNP_HIP_SCALAR_FORESTS: *value = s[kStatForests]; break;
    case AGBNP_HIP_SCALAR_ROWS_ON: *value = c->P.rows_on; break;
    case AGBNP_HIP_SCALAR_ROW_BUILDS: *value = c->last_rows[kNlBuilds]; break;
    case AGBNP_HIP_SCALAR_PACK_LEVEL: *value = c->last_pack[kPsLevel]; break;
    case AGBNP_HIP_SCALAR_PACK_AGE: *value = c->last_pack[kPsAge]; break;
    case AGBNP_HIP_SCALAR_ROW_SLICE: *value = c->last_rows[kNlSlice]; break;
    case AGBNP_HIP_SCALAR_PACK_PLANS: *value = c->last_pack[kPsPlans]; break;
    case AGBNP_HIP_SCALAR_LAUNCHES: *value = c->version == 1 ? (c->five_active ? 5 : 6) : (c->five_active ? 2 : 3); break;  // (no k_prep launch in the five-launch mode)
    default: return c->fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, "unknown scalar id");
  }
  return AGBNP_HIP_OK;
}

int agbnp_hip_get_vector(agbnp_hip_context* c, int which, double* out) {
  if (!c || !out) return AGBNP_HIP_ERR_INVALID_ARGUMENT;
  const int rc_ = catch_up(c);
  if (rc_ != AGBNP_HIP_OK) return rc_;
  if (!c->have_results) return c->fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, "no completed evaluation yet");
  HIP_TRY(c, hipSetDevice(c->device));
  const int n = c->n, nh = c->nh;
  auto heavy_to_atoms = [&](const double* dsrc, size_t stride, size_t word, double scale_by_inv_vol) -> int {
    std::vector<double> raw(c->nhp() * stride);
    HIP_TRY(c, hipMemcpy(raw.data(), dsrc, sizeof(double) * raw.size(), hipMemcpyDeviceToHost));
    for (int i = 0; i < n; i++) out[i] = 0.0;
    for (int h = 0; h < nh; h++) {
      double v = raw[(size_t)h * stride + word];
      if (scale_by_inv_vol != 0.0) v /= (4. * M_PI * pow(c->r_vdw[c->h2a[h]], 3) / 3.);
      out[c->h2a[h]] = v;
    }
    return AGBNP_HIP_OK;
  };
  switch (which) {
    case AGBNP_HIP_VECTOR_SELFVOL_VDW: return heavy_to_atoms(c->hrow(kHvSvVdw), 1, 0, 0.0);
    case AGBNP_HIP_VECTOR_BORN:
      if (c->version != 1) return c->fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, "Born radii exist for version 1 only");
      HIP_TRY(c, hipMemcpy(out, c->P.born, sizeof(double) * n, hipMemcpyDeviceToHost));
      return AGBNP_HIP_OK;
    case AGBNP_HIP_VECTOR_SCALE: return heavy_to_atoms(c->hrow(kHvSvVdw), 1, 0, 1.0);
    case AGBNP_HIP_VECTOR_SELFVOL_LARGE:
      if (!c->diagnostics) return c->fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, "enlarged-radius self volumes need agbnp_hip_set_diagnostics(ctx, 1) before the evaluation");
      return heavy_to_atoms(c->hrow(kHvSvLarge), 1, 0, 0.0);
    case AGBNP_HIP_VECTOR_SUBTREE_NODES:
    case AGBNP_HIP_VECTOR_SUBTREE_ATOMS: {  // overlap-tree shape: nodes / local atoms of the subtree rooted at every heavy atom (0 for hydrogens)
      std::vector<int2> sz(c->nhp());
      HIP_TRY(c, hipMemcpy(sz.data(), c->sizes(c->set_held()), sizeof(int2) * c->nhp(), hipMemcpyDeviceToHost));
      for (int i = 0; i < n; i++) out[i] = 0.0;
      for (int h = 0; h < nh; h++) out[c->h2a[h]] = which == AGBNP_HIP_VECTOR_SUBTREE_NODES ? sz[h].x : sz[h].y;
      return AGBNP_HIP_OK;
    }
    default: return c->fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, "unknown vector id");
  }
}

int agbnp_hip_get_table_sizes(agbnp_hip_context* c, int* nscreened, int* nscreener) {
  if (!c || !nscreened || !nscreener) return AGBNP_HIP_ERR_INVALID_ARGUMENT;
  *nscreened = c->lut.nscreened;
  *nscreener = c->lut.nscreener;
  return AGBNP_HIP_OK;
}

int agbnp_hip_get_tables(agbnp_hip_context* c, double* y, double* y2, int* type_screened, int* type_screener) {
  if (!c || !y || !y2 || !type_screened || !type_screener) return AGBNP_HIP_ERR_INVALID_ARGUMENT;
  memcpy(y, c->lut.y.data(), sizeof(double) * c->lut.y.size());
  memcpy(y2, c->lut.y2.data(), sizeof(double) * c->lut.y2.size());
  memcpy(type_screened, c->lut.type_screened.data(), sizeof(int) * c->n);
  memcpy(type_screener, c->lut.type_screener.data(), sizeof(int) * c->n);
  return AGBNP_HIP_OK;
}

int agbnp_hip_get_mode(const agbnp_hip_context* c) { return c ? c->mode : -1; }

int agbnp_hip_set_profiling(agbnp_hip_context* c, int enabled) {
  if (!c) return AGBNP_HIP_ERR_INVALID_ARGUMENT;
  c->timeline.enabled = enabled != 0;
  c->timeline.used = 0;
  for (int k = 0; k < kKernelCount; k++) {
    c->kernel_ms[k] = 0.0;
    c->kernel_launches[k] = 0;
  }
  return AGBNP_HIP_OK;
}

int agbnp_hip_num_kernels(void) { return kKernelCount; }

const char* agbnp_hip_kernel_name(int index) {
  static const char* names[kKernelCount] = {"k_prep",        "k_tree_cavity", "k_born_tiles", "k_gb_tiles", "k_dborn_tiles",
                                            "k_tree_pseudo", "k_outputs",     "k_born_rows",  "k_dborn_rows",  "k_gb_rows",
                                            "k_energy_roles", "k_decompose",  "k_pair_matrix"};
  return (index >= 0 && index < kKernelCount) ? names[index] : "";
}

int agbnp_hip_get_kernel_times(agbnp_hip_context* c, double* total_ms, long* launches) {
  if (!c || !total_ms || !launches) return AGBNP_HIP_ERR_INVALID_ARGUMENT;
  for (int k = 0; k < kKernelCount; k++) {
    total_ms[k] = c->kernel_ms[k];
    launches[k] = c->kernel_launches[k];
  }
  return AGBNP_HIP_OK;
}

int agbnp_hip_host_tables(int n, const double* radius, const int* ishydrogen, int* nscreened, int* nscreener, double* y,
                          double* y2, int table_capacity, int* type_screened, int* type_screener) {
  if (n <= 0 || !radius || !ishydrogen || !nscreened || !nscreener || !y || !y2 || !type_screened || !type_screener) {
    g_create_error = "agbnp_hip_host_tables: null pointer or non-positive particle count";
    return AGBNP_HIP_ERR_INVALID_ARGUMENT;
  }
  I4TableSet t;
  t.build(std::vector<double>(radius, radius + n), std::vector<int>(ishydrogen, ishydrogen + n));
  *nscreened = t.nscreened;
  *nscreener = t.nscreener;
  if ((int)t.y.size() > table_capacity) {
    g_create_error = "agbnp_hip_host_tables: table_capacity too small";
    return AGBNP_HIP_ERR_INVALID_ARGUMENT;
  }
  memcpy(y, t.y.data(), sizeof(double) * t.y.size());
  memcpy(y2, t.y2.data(), sizeof(double) * t.y2.size());
  memcpy(type_screened, t.type_screened.data(), sizeof(int) * n);
  memcpy(type_screener, t.type_screener.data(), sizeof(int) * n);
  return AGBNP_HIP_OK;
}

int agbnp_hip_withheld_evaluations(const agbnp_hip_context* c, int* indices, int capacity) {
  if (!c) return -1;
  for (int k = 0; indices && k < capacity && k < (int)c->withheld.size(); k++) indices[k] = c->withheld[k];
  return c->withheld_count;
}

unsigned agbnp_hip_generation(const agbnp_hip_context* c) { return c ? c->generation : 0u; }

// ---- diagnostic entry points (not part of include/agbnp_hip.h; used by scripts/ only) ---------------------------------
// the forest packing as the device holds it, in WORK-SLOT order: the items of slot s at forest_start[s] .. forest_start[s+1]),
// and the per-subtree shapes
int agbnp_debug_get_packing(agbnp_hip_context* c, int* order, int order_cap, int* forest_start, int start_cap, int* nforests, int* sizes) {
  if (!c) return AGBNP_HIP_ERR_INVALID_ARGUMENT;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipDeviceSynchronize());
  int nf = 0;
  HIP_TRY(c, hipMemcpy(&nf, c->d_forest.p + c->slot_cap + kPackForestsNext, sizeof(int), hipMemcpyDeviceToHost));
  nf = std::min(nf, c->slot_cap);
  *nforests = nf;
  std::vector<int> rows(c->d_rows.count);
  HIP_TRY(c, hipMemcpy(rows.data(), c->d_rows.p, sizeof(int) * rows.size(), hipMemcpyDeviceToHost));
  int run = 0;
  for (int s = 0; s < nf && s + 1 < start_cap; s++) {
    forest_start[s] = run;
    for (int k = 0; k < rows[slot_row_count(s)] && run < order_cap; k++) order[run++] = rows[slot_row_item(s, k)];
    forest_start[s + 1] = run;
  }
  if (sizes) HIP_TRY(c, hipMemcpy(sizes, c->sizes(c->set_held()), sizeof(int2) * c->nhp(), hipMemcpyDeviceToHost));
  return AGBNP_HIP_OK;
}
// replaces the packing (same form) and (freeze != 0) stops the bookkeeping from planning new ones
int agbnp_debug_set_packing(agbnp_hip_context* c, const int* order, int norder, const int* forest_start, int nforests, int freeze) {
  if (!c) return AGBNP_HIP_ERR_INVALID_ARGUMENT;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipDeviceSynchronize());
  if (order) {
    if (nforests > c->slot_cap) return c->fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, "agbnp_debug_set_packing: more forests than work slots");
    std::vector<int> rows(c->d_rows.count, -1);
    for (int s = 0; s < nforests; s++) {
      const int count = std::min(forest_start[s + 1] - forest_start[s], (int)kMaxItems);
      rows[slot_row_count(s)] = count;
      for (int k = 0; k < count && forest_start[s] + k < norder; k++) rows[slot_row_item(s, k)] = order[forest_start[s] + k];
    }
    HIP_TRY(c, hipMemcpy(c->d_rows.p, rows.data(), sizeof(int) * rows.size(), hipMemcpyHostToDevice));
    if (c->five) {  // (five-launch mode: the roots' atoms beside the rows)
      std::vector<int> atoms((size_t)kMaxItems * c->slot_cap, 0);
      bool roots_exist = true;
      for (int s = 0; s < nforests; s++)
        for (int k = 0; k < kMaxItems; k++) {
          const int item = rows[slot_row_item(s, k)];
          if (item >= 0 && work_item_root(item) < c->nh) atoms[(size_t)kMaxItems * s + k] = c->h2a[work_item_root(item)];
          if (item >= 0 && work_item_root(item) >= c->nh) roots_exist = false;
        }
      HIP_TRY(c, hipMemcpy(c->d_row_atoms.p, atoms.data(), sizeof(int) * atoms.size(), hipMemcpyHostToDevice));
      // (a context that runs through agbnp_hip_execute_openmm keeps its kind: the slots of the new rows' roots, as enqueue would
      // write them -- the hook replaces a packing, it does not make captured graphs stale)
      if (c->row_atoms_kind == 1 && roots_exist) {  // (k_row_atoms reads the map at every root it is given)
        HIP_TRY(c, launch_row_atoms(c->slot_cap, c->d_rows.p, c->d_hslot.p, c->d_row_atoms.p, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
      } else if (c->row_atoms_kind == 1) {
        set_row_atoms_kind(c, -1);
      }  // (-1: enqueue rewrites them anyway)
    }
    HIP_TRY(c, hipMemcpy(c->d_forest.p + c->slot_cap + kPackForestsNext, &nforests, sizeof(int), hipMemcpyHostToDevice));
  }
  c->P.pack_enabled = freeze ? 3 : c->P.pack_enabled;  // 3: the bookkeeping keeps its statistics but writes no packing
  return AGBNP_HIP_OK;
}

// row form: bw_i = brw_i + bru_i as the GB stage left it [n], W+U by heavy index [nh] (what the chain-rule stage left)
int agbnp_debug_get_rows(agbnp_hip_context* c, double* bw, double* wu) {
  if (!c || !c->rows_capable) return AGBNP_HIP_ERR_INVALID_ARGUMENT;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipDeviceSynchronize());
  HIP_TRY(c, hipMemcpy(bw, c->P.bw, sizeof(double) * c->n, hipMemcpyDeviceToHost));
  HIP_TRY(c, hipMemcpy(wu, c->P.db_wu, sizeof(double) * c->nh, hipMemcpyDeviceToHost));
  return AGBNP_HIP_OK;
}

int agbnp_hip_num_particles(const agbnp_hip_context* c) { return c ? c->n : -1; }
int agbnp_hip_version(const agbnp_hip_context* c) { return c ? c->version : -1; }

}  // extern "C"
