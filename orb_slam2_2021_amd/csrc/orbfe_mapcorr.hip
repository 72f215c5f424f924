// orbfe_mapcorr.hip -- the map corrections on the GPU (include/orbfe_mapcorr.h): UpdateNormalAndDepth,
// CorrectLoop's pose and point correction, RunGlobalBundleAdjustment's map update. The arithmetic is
// orbfe_mapcorr_core.h's, one item per thread:
//   k_mc_normals     call 1: one thread per point over its observers (a sequential float chain by
//                    definition, about 8 long); the centres are 12 bytes per keyframe and stay in L2
//   k_mc_centres     call 2: one thread per keyframe: the old camera centres
//   k_mc_loop_kf     call 2: one thread per list position: the two Sim3, the inverse, the pose, the new centre
//   k_mc_loop_mark   call 2: one thread per row slot: atomicMin of the list position into the slot's point.
//                    A minimum: nothing depends on the order of the atomics.
//   k_mc_loop_point  call 2: one thread per point: the correction, then UpdateNormalAndDepth
//   k_mc_gba_kf      call 3: one launch per level of orbfe_mapcorr_core.h's plan, one thread per keyframe of
//                    the level; the stream orders the levels
//   k_mc_gba_point   call 3: one thread per point
// A call packs its inputs into the handle's pinned block, uploads it in one copy, launches, and reads
// the outputs back in one copy with one synchronisation. Every index a kernel reads was checked on
// the host before anything is uploaded; every loop runs to a count among those.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/orbfe_mapcorr.h"
#include "orbfe_device.h"
#include "orbfe_ktimer.h"
#include "orbfe_mapcorr_core.h"
#include "orbfe_stage.h"

#define MC_BLOCK 256

__global__ __launch_bounds__(MC_BLOCK) void k_mc_normals(McNd w, const float* xw, const uint8_t* bad, int n_points) {
  const int p = blockIdx.x * MC_BLOCK + threadIdx.x;
  if (p < n_points) mc_nd_point(w, xw, bad, p);
}

__global__ __launch_bounds__(MC_BLOCK) void k_mc_centres(const float* tcw, float* ow, int n_kf) {
  const int k = blockIdx.x * MC_BLOCK + threadIdx.x;
  if (k < n_kf) mc_centre(tcw + 12 * (size_t)k, ow + 3 * (size_t)k);
}

__global__ __launch_bounds__(MC_BLOCK) void k_mc_loop_kf(McLoop w) {
  const int i = blockIdx.x * MC_BLOCK + threadIdx.x;
  if (i < w.n_connected) mc_loop_kf(w, i);
}

__global__ __launch_bounds__(MC_BLOCK) void k_mc_loop_mark(McLoop w) {
  const int t = blockIdx.x * MC_BLOCK + threadIdx.x;
  if (t < w.n_slots) mc_loop_mark(w, t);
}

__global__ __launch_bounds__(MC_BLOCK) void k_mc_loop_point(McLoop w) {
  const int p = blockIdx.x * MC_BLOCK + threadIdx.x;
  if (p < w.n_points) mc_loop_point(w, p);
}

__global__ __launch_bounds__(MC_BLOCK) void k_mc_gba_kf(McGba w, int begin, int end) {
  const int i = begin + blockIdx.x * MC_BLOCK + threadIdx.x;
  if (i < end) mc_gba_kf(w, w.order[i]);
}

__global__ __launch_bounds__(MC_BLOCK) void k_mc_gba_point(McGba w) {
  const int p = blockIdx.x * MC_BLOCK + threadIdx.x;
  if (p < w.n_points) mc_gba_point(w, p);
}

// ------------------------------------------------------------------------------------------
// host

struct orbfe_mapcorr : OrbfeDev {
  int max_kf = 0, max_points = 0, max_edges = 0;
  OrbfeStage in, out;      // inputs (one upload), outputs (one copy back)
  uint8_t* d_work = nullptr;  // device only: the old and new centres, the inverses
  size_t work_bytes = 0;
};

namespace {
const int MC_ARRAYS = 32;  // more than the arrays any block holds: the alignment's share

// the largest input block any of the three calls packs
size_t mc_in_bytes(size_t nk, size_t np, size_t ne) {
  const size_t per_kf = 12 * 4 * 2 + 3 * 4 + 1 + 4 * 5, per_pt = 12 * 2 + 1 * 2 + 4 * 3 + 4, per_edge = 4 * 2;
  return per_kf * (nk + 1) + per_pt * (np + 1) + per_edge * ne + 4 * ORBFE_MAPCORR_MAX_LEVELS + 256 * MC_ARRAYS;
}
size_t mc_out_bytes(size_t nk, size_t np) {
  return (8 * 8 * 2 + 12 * 4) * nk + (12 + 4 + 12 + 4 + 4 + 1 + 1) * np + 256 * MC_ARRAYS;
}
size_t mc_work_bytes(size_t nk) { return (3 * 4 * 2 + 8 * 8) * nk + 256 * MC_ARRAYS; }

unsigned mc_grid(long long n) { return (unsigned)((n + MC_BLOCK - 1) / MC_BLOCK); }

struct McErr {
  const char* who;
  int operator()(int st, const char* what) const {
    char msg[160];
    snprintf(msg, sizeof(msg), "%s: %s", who, what);
    return orbfe_set_error(st, msg);
  }
};

// the points' side of a problem; loop: the points that CorrectLoop may update are not known before the
// marks, so every point that is not bad and has an observer is held to the ref_kf / ref_level rule
int mc_check_points(const McErr& err, const orbfe_mapcorr* h, int n_kf, const orbfe_mapcorr_points_t& q,
                    const orbfe_mapcorr_normals_t& r) {
  if (q.n_points < 0 || q.n_obs < 0) return err(ORBFE_ERR_ARG, "negative count");
  if (q.n_points > h->max_points || q.n_obs > h->max_edges) return err(ORBFE_ERR_CAPACITY, "problem above the handle's bounds");
  if (q.n_levels < 1 || q.n_levels > ORBFE_MAPCORR_MAX_LEVELS) return err(ORBFE_ERR_ARG, "n_levels outside 1..64");
  if (!q.scale_factors || !q.obs_begin || (q.n_obs > 0 && !q.obs_kf) ||
      (q.n_points > 0 && (!q.xw || !q.bad || !q.ref_kf || !q.ref_level || !r.normal || !r.max_dist || !r.min_dist || !r.updated)))
    return err(ORBFE_ERR_ARG, "null array");
  if (q.obs_begin[0] != 0 || q.obs_begin[q.n_points] != q.n_obs) return err(ORBFE_ERR_ARG, "obs_begin is not a CSR over n_obs");
  for (int p = 0; p < q.n_points; p++) {
    const int b = q.obs_begin[p], e = q.obs_begin[p + 1];
    if (b > e || b < 0 || e > q.n_obs) return err(ORBFE_ERR_ARG, "obs_begin is not a CSR over n_obs");
    if (!q.bad[p] && e > b) {
      if (q.ref_kf[p] < 0 || q.ref_kf[p] >= n_kf) return err(ORBFE_ERR_ARG, "reference keyframe index out of range");
      if (q.ref_level[p] < 0 || q.ref_level[p] >= q.n_levels) return err(ORBFE_ERR_ARG, "ref_level outside 0..n_levels-1");
    }
  }
  for (int i = 0; i < q.n_obs; i++)
    if (q.obs_kf[i] < 0 || q.obs_kf[i] >= n_kf) return err(ORBFE_ERR_ARG, "observing keyframe index out of range");
  return ORBFE_OK;
}

// packs the points' side into the input block and lays the normals out in the output block
struct McNormalsHost {
  float *normal, *max_dist, *min_dist;
  uint8_t* updated;
};

void mc_pack_points(orbfe_mapcorr* h, const orbfe_mapcorr_points_t& q, McNd* nd, const float** d_xw, const uint8_t** d_bad,
                    McNormalsHost* host) {
  const size_t np = q.n_points;
  nd->scale = h->in.put(q.scale_factors, q.n_levels);
  nd->n_levels = q.n_levels;
  *d_xw = h->in.put(q.xw, 3 * np);
  *d_bad = h->in.put(q.bad, np);
  nd->obs_begin = h->in.put(q.obs_begin, np + 1);
  nd->obs_kf = h->in.put(q.obs_kf, q.n_obs);
  nd->ref_kf = h->in.put(q.ref_kf, np);
  nd->ref_level = h->in.put(q.ref_level, np);
  nd->normal = h->out.take<float>(3 * np, &host->normal);
  nd->max_dist = h->out.take<float>(np, &host->max_dist);
  nd->min_dist = h->out.take<float>(np, &host->min_dist);
  nd->updated = h->out.take<uint8_t>(np, &host->updated);
}

// in/out: the caller's three arrays are written only where the point was updated
void mc_unpack_normals(const McNormalsHost& host, int n_points, const orbfe_mapcorr_normals_t& r) {
  for (int p = 0; p < n_points; p++) {
    r.updated[p] = host.updated[p];
    if (!host.updated[p]) continue;
    for (int c = 0; c < 3; c++) r.normal[3 * (size_t)p + c] = host.normal[3 * (size_t)p + c];
    r.max_dist[p] = host.max_dist[p];
    r.min_dist[p] = host.min_dist[p];
  }
}

}  // namespace

extern "C" int orbfe_mapcorr_create(int device, int max_kf, int max_points, int max_edges, orbfe_mapcorr** out) {
  if (!out) return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_mapcorr_create: bad argument");
  *out = nullptr;
  if (max_kf < 1 || max_kf > ORBFE_MAPCORR_MAX_KF || max_points < 1 || max_points > ORBFE_MAPCORR_MAX_POINTS || max_edges < 1 ||
      max_edges > ORBFE_MAPCORR_MAX_EDGES)
    return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_mapcorr_create: max_kf in 1..8192, max_points in 1..1048576, max_edges in 1..16777216");
  orbfe_mapcorr* h = new orbfe_mapcorr();
  h->max_kf = max_kf, h->max_points = max_points, h->max_edges = max_edges;
  if (device < 0) {
    *out = h;
    return ORBFE_OK;
  }
  const int open_st = orbfe_dev_open(h, device, "orbfe_mapcorr_create");
  if (open_st != ORBFE_OK) {
    orbfe_mapcorr_destroy(h);
    return open_st;
  }
  h->work_bytes = mc_work_bytes(max_kf);
  ORBFE_CREATE_HIP(h, orbfe_mapcorr_destroy, orbfe_stage_alloc(&h->in, mc_in_bytes(max_kf, max_points, max_edges), true));
  ORBFE_CREATE_HIP(h, orbfe_mapcorr_destroy, orbfe_stage_alloc(&h->out, mc_out_bytes(max_kf, max_points), true));
  ORBFE_CREATE_HIP(h, orbfe_mapcorr_destroy, hipMalloc(&h->d_work, h->work_bytes));
  *out = h;
  return ORBFE_OK;
}

extern "C" int orbfe_mapcorr_destroy(orbfe_mapcorr* h) {
  if (!h) return ORBFE_OK;
  if (orbfe_dev_close(h)) {
    orbfe_stage_free(&h->in);
    orbfe_stage_free(&h->out);
    hipFree(h->d_work);
  }
  delete h;
  return ORBFE_OK;
}

extern "C" int orbfe_mapcorr_update_normal_depth(orbfe_mapcorr* h, const orbfe_mapcorr_normals_problem_t* p,
                                                 orbfe_mapcorr_normals_t* r) {
  if (!h || !p || !r) return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_mapcorr_update_normal_depth: bad argument");
  const McErr err = {"orbfe_mapcorr_update_normal_depth"};
  if (p->n_kf < 0) return err(ORBFE_ERR_ARG, "negative count");
  if (p->n_kf > h->max_kf) return err(ORBFE_ERR_CAPACITY, "problem above the handle's bounds");
  if (p->n_kf > 0 && !p->ow) return err(ORBFE_ERR_ARG, "null array");
  const orbfe_mapcorr_points_t& q = p->points;
  int st = mc_check_points(err, h, p->n_kf, q, *r);
  if (st != ORBFE_OK) return st;
  if (h->device < 0) return orbfe_set_error(ORBFE_ERR_STATE, "map corrector is host-only (device < 0)");
  ORBFE_HIP_CHECK(hipSetDevice(h->device));
  h->in.off = h->out.off = 0;
  McNd nd;
  memset(&nd, 0, sizeof(nd));
  const float* d_xw;
  const uint8_t* d_bad;
  McNormalsHost host;
  nd.ow = h->in.put(p->ow, 3 * (size_t)p->n_kf);
  mc_pack_points(h, q, &nd, &d_xw, &d_bad, &host);
  if ((st = orbfe_stage_upload(&h->in, h->stream)) != ORBFE_OK) return st;
  if (q.n_points > 0)
    ORBFE_LAUNCH("k_mc_normals", k_mc_normals, dim3(mc_grid(q.n_points)), dim3(MC_BLOCK), 0, h->stream, nd, d_xw, d_bad, q.n_points);
  if ((st = orbfe_stage_download(&h->out, h->stream)) != ORBFE_OK) return st;
  mc_unpack_normals(host, q.n_points, *r);
  return ORBFE_OK;
}

extern "C" int orbfe_mapcorr_correct_loop(orbfe_mapcorr* h, const orbfe_mapcorr_loop_problem_t* p, orbfe_mapcorr_loop_result_t* r) {
  if (!h || !p || !r) return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_mapcorr_correct_loop: bad argument");
  const McErr err = {"orbfe_mapcorr_correct_loop"};
  const orbfe_mapcorr_points_t& q = p->points;
  if (p->n_kf < 0 || p->n_connected < 0 || p->n_slots < 0) return err(ORBFE_ERR_ARG, "negative count");
  if (p->n_kf > h->max_kf || p->n_slots > h->max_edges) return err(ORBFE_ERR_CAPACITY, "problem above the handle's bounds");
  if (p->n_connected < 1 || p->n_connected > p->n_kf) return err(ORBFE_ERR_ARG, "n_connected outside 1..n_kf");
  if (!p->tcw || !p->connected_kf || !p->scw || !p->row_begin || (p->n_slots > 0 && !p->row_point) || !r->noncorrected_sim3 ||
      !r->corrected_sim3 || !r->tcw_out)
    return err(ORBFE_ERR_ARG, "null array");
  int st = mc_check_points(err, h, p->n_kf, q, r->normals);
  if (st != ORBFE_OK) return st;
  if (q.n_points > 0 && (!r->xw_out || !r->corrected_by)) return err(ORBFE_ERR_ARG, "null array");
  if (p->cur < 0 || p->cur >= p->n_connected) return err(ORBFE_ERR_ARG, "cur outside the connected list");
  std::vector<int> pos_of_kf(p->n_kf, -1);
  for (int i = 0; i < p->n_connected; i++) {
    const int k = p->connected_kf[i];
    if (k < 0 || k >= p->n_kf) return err(ORBFE_ERR_ARG, "connected keyframe index out of range");
    if (pos_of_kf[k] >= 0) return err(ORBFE_ERR_ARG, "a connected keyframe listed twice");
    pos_of_kf[k] = i;
  }
  if (p->row_begin[0] != 0 || p->row_begin[p->n_connected] != p->n_slots) return err(ORBFE_ERR_ARG, "row_begin is not a CSR over n_slots");
  for (int i = 0; i < p->n_connected; i++)
    if (p->row_begin[i] > p->row_begin[i + 1] || p->row_begin[i] < 0 || p->row_begin[i + 1] > p->n_slots)
      return err(ORBFE_ERR_ARG, "row_begin is not a CSR over n_slots");
  for (int t = 0; t < p->n_slots; t++)
    if (p->row_point[t] < -1 || p->row_point[t] >= q.n_points) return err(ORBFE_ERR_ARG, "row point index out of range");
  if (h->device < 0) return orbfe_set_error(ORBFE_ERR_STATE, "map corrector is host-only (device < 0)");
  ORBFE_HIP_CHECK(hipSetDevice(h->device));

  h->in.off = h->out.off = 0;
  const size_t nk = p->n_kf, nc = p->n_connected, np = q.n_points;
  McLoop w;
  memset(&w, 0, sizeof(w));
  w.n_kf = p->n_kf, w.n_connected = p->n_connected, w.cur = p->cur, w.n_points = q.n_points, w.n_slots = p->n_slots;
  memcpy(w.scw, p->scw, sizeof(w.scw));
  w.tcw = h->in.put(p->tcw, 12 * nk);
  w.connected_kf = h->in.put(p->connected_kf, nc);
  w.nd.pos_of_kf = h->in.put(pos_of_kf.data(), nk);
  w.row_begin = h->in.put(p->row_begin, nc + 1);
  w.row_point = h->in.put(p->row_point, p->n_slots);
  McNormalsHost host;
  mc_pack_points(h, q, &w.nd, &w.xw, &w.bad, &host);
  double *h_nonc, *h_corr;
  float *h_tcw, *h_xw;
  int* h_by;
  w.nonc = h->out.take<double>(8 * nc, &h_nonc);
  w.corr = h->out.take<double>(8 * nc, &h_corr);
  w.tcw_out = h->out.take<float>(12 * nc, &h_tcw);
  w.xw_out = h->out.take<float>(3 * np, &h_xw);
  w.corrected_by = h->out.take<int>(np, &h_by);
  OrbfeStage work;
  work.d = h->d_work;
  w.ow_old = work.take<float>(3 * nk, nullptr);
  w.ow_new = work.take<float>(3 * nc, nullptr);
  w.swi = work.take<double>(8 * nc, nullptr);
  w.nd.ow = w.ow_old, w.nd.ow_new = w.ow_new;

  if ((st = orbfe_stage_upload(&h->in, h->stream)) != ORBFE_OK) return st;
  ORBFE_LAUNCH("k_mc_centres", k_mc_centres, dim3(mc_grid(p->n_kf)), dim3(MC_BLOCK), 0, h->stream, w.tcw, w.ow_old, p->n_kf);
  ORBFE_LAUNCH("k_mc_loop_kf", k_mc_loop_kf, dim3(mc_grid(p->n_connected)), dim3(MC_BLOCK), 0, h->stream, w);
  if (np > 0) {
    ORBFE_HIP_CHECK(hipMemsetAsync(w.corrected_by, 0x7f, sizeof(int) * np, h->stream));  // MC_NONE
    if (p->n_slots > 0)
      ORBFE_LAUNCH("k_mc_loop_mark", k_mc_loop_mark, dim3(mc_grid(p->n_slots)), dim3(MC_BLOCK), 0, h->stream, w);
    ORBFE_LAUNCH("k_mc_loop_point", k_mc_loop_point, dim3(mc_grid(q.n_points)), dim3(MC_BLOCK), 0, h->stream, w);
  }
  if ((st = orbfe_stage_download(&h->out, h->stream)) != ORBFE_OK) return st;
  memcpy(r->noncorrected_sim3, h_nonc, sizeof(double) * 8 * nc);
  memcpy(r->corrected_sim3, h_corr, sizeof(double) * 8 * nc);
  memcpy(r->tcw_out, h_tcw, sizeof(float) * 12 * nc);
  if (np > 0) {
    memcpy(r->xw_out, h_xw, sizeof(float) * 3 * np);
    memcpy(r->corrected_by, h_by, sizeof(int) * np);
  }
  mc_unpack_normals(host, q.n_points, r->normals);
  return ORBFE_OK;
}

extern "C" int orbfe_mapcorr_apply_gba(orbfe_mapcorr* h, const orbfe_mapcorr_gba_problem_t* p, orbfe_mapcorr_gba_result_t* r) {
  if (!h || !p || !r) return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_mapcorr_apply_gba: bad argument");
  const McErr err = {"orbfe_mapcorr_apply_gba"};
  if (p->n_kf < 0 || p->n_points < 0) return err(ORBFE_ERR_ARG, "negative count");
  if (p->n_kf > h->max_kf || p->n_points > h->max_points) return err(ORBFE_ERR_CAPACITY, "problem above the handle's bounds");
  if ((p->n_kf > 0 && (!p->tcw || !p->tcw_gba || !p->optimised || !p->parent || !r->tcw_out || !r->propagated)) ||
      (p->n_points > 0 && (!p->xw || !p->bad || !p->pt_optimised || !p->xw_gba || !p->ref_kf || !r->xw_out || !r->pt_changed)))
    return err(ORBFE_ERR_ARG, "null array");
  McGbaPlan plan;
  switch (mc_gba_plan(p->n_kf, p->parent, p->optimised, &plan)) {
    case MC_PLAN_PARENT: return err(ORBFE_ERR_ARG, "parent index out of range");
    case MC_PLAN_CYCLE: return err(ORBFE_ERR_ARG, "the parents form a cycle");
    case MC_PLAN_ORIGIN: return err(ORBFE_ERR_ARG, "an origin is not optimised");
    default: break;
  }
  for (int q = 0; q < p->n_points; q++)
    if (p->ref_kf[q] < -1 || p->ref_kf[q] >= p->n_kf) return err(ORBFE_ERR_ARG, "reference keyframe index out of range");
  if (h->device < 0) return orbfe_set_error(ORBFE_ERR_STATE, "map corrector is host-only (device < 0)");
  ORBFE_HIP_CHECK(hipSetDevice(h->device));

  h->in.off = h->out.off = 0;
  const size_t nk = p->n_kf, np = p->n_points;
  McGba w;
  memset(&w, 0, sizeof(w));
  w.n_kf = p->n_kf, w.n_points = p->n_points;
  w.tcw = h->in.put(p->tcw, 12 * nk);
  w.tcw_gba = h->in.put(p->tcw_gba, 12 * nk);
  w.optimised = h->in.put(p->optimised, nk);
  w.parent = h->in.put(p->parent, nk);
  w.order = h->in.put(plan.order.data(), nk);
  w.xw = h->in.put(p->xw, 3 * np);
  w.bad = h->in.put(p->bad, np);
  w.pt_optimised = h->in.put(p->pt_optimised, np);
  w.xw_gba = h->in.put(p->xw_gba, 3 * np);
  w.ref_kf = h->in.put(p->ref_kf, np);
  float *h_tcw, *h_xw;
  uint8_t* h_changed;
  w.tcw_out = h->out.take<float>(12 * nk, &h_tcw);
  w.xw_out = h->out.take<float>(3 * np, &h_xw);
  w.pt_changed = h->out.take<uint8_t>(np, &h_changed);
  OrbfeStage work;
  work.d = h->d_work;
  w.ow_out = work.take<float>(3 * nk, nullptr);

  int st;
  if ((st = orbfe_stage_upload(&h->in, h->stream)) != ORBFE_OK) return st;
  const int levels = (int)plan.level_begin.size() - 1;
  for (int d = 0; d < levels; d++) {
    const int b = plan.level_begin[d], e = plan.level_begin[d + 1];
    if (e > b) ORBFE_LAUNCH("k_mc_gba_kf", k_mc_gba_kf, dim3(mc_grid(e - b)), dim3(MC_BLOCK), 0, h->stream, w, b, e);
  }
  if (np > 0) ORBFE_LAUNCH("k_mc_gba_point", k_mc_gba_point, dim3(mc_grid(p->n_points)), dim3(MC_BLOCK), 0, h->stream, w);
  if ((st = orbfe_stage_download(&h->out, h->stream)) != ORBFE_OK) return st;
  if (nk > 0) memcpy(r->tcw_out, h_tcw, sizeof(float) * 12 * nk);
  for (size_t k = 0; k < nk; k++) r->propagated[k] = p->optimised[k] ? 0 : 1;
  if (np > 0) {
    memcpy(r->xw_out, h_xw, sizeof(float) * 3 * np);
    memcpy(r->pt_changed, h_changed, np);
  }
  r->levels = levels;
  return ORBFE_OK;
}
