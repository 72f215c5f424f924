// orbfe_poseopt.hip -- Optimizer::PoseOptimization on the GPU (include/orbfe_poseopt.h): a batch of
// motion-only Levenberg-Marquardt problems, one wavefront each.
//
//   k_poseopt  one block of 64 lanes per problem: the lanes stride the frame's keypoints, the sums of
//              H, b and chi2 cross the lanes by the fixed shuffle tree, lane 0 factors the 6x6 system
//              in LDS, and the four rounds with their classifications run inside the one launch
//
// One call stages every problem in one pinned buffer (one H2D copy), launches once on the handle's
// stream and takes every result down in one D2H copy. All offsets are formed on the host from counts
// it has checked against the handle's bounds; the kernel indexes the arrays only with i < n from its
// strided loops. The outlier flags of a lane's edges are the bits of one 64-bit register (max_obs <=
// 64 * 64) and an edge's stale error is recomputed from the last evaluated pose, so the kernel needs
// no per-edge workspace.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>

#include "../../include/orbfe_poseopt.h"
#include "orbfe_device.h"
#include "orbfe_ktimer.h"
#include "orbfe_lm_device.h"
#include "orbfe_poseopt_core.h"
#include "orbfe_stage.h"

static_assert(LM_FLAG_LARGE_STEP == ORBFE_POSEOPT_FLAG_LARGE_STEP && LM_FLAG_NONFINITE == ORBFE_POSEOPT_FLAG_NONFINITE,
              "flag values");
static_assert(LM_STOP_ALL == ORBFE_POSEOPT_STOP_ALL && LM_STOP_TERMINATE == ORBFE_POSEOPT_STOP_TERMINATE &&
                  LM_STOP_NBAD == ORBFE_POSEOPT_STOP_NBAD && LM_STOP_NO_EDGE == ORBFE_POSEOPT_STOP_NO_EDGE,
              "stop codes");
static_assert(ORBFE_POSEOPT_MAX_OBS <= PO_LANES * 64, "a lane's outlier flags are one 64-bit word");
static_assert(sizeof(PoRound) == sizeof(orbfe_poseopt_round_t), "trace layout");

__global__ __launch_bounds__(PO_LANES) void k_poseopt(const uint8_t* __restrict__ in, uint8_t* __restrict__ res) {
  const PoDev& D = reinterpret_cast<const PoDev*>(in)[blockIdx.x];
  __shared__ PoWork work;
  __shared__ double red[PO_ACC];
  PoProblem P;
  P.n = D.n;
  P.valid = in + D.in_valid;
  P.xw = reinterpret_cast<const float*>(in + D.in_xw);
  P.kp = reinterpret_cast<const float*>(in + D.in_kp);
  P.ur = reinterpret_cast<const float*>(in + D.in_ur);
  P.inv_sigma2 = reinterpret_cast<const float*>(in + D.in_is2);
  // the camera and the start pose go through LDS for the same reason as the sums (LmDevGroup::reduce)
  __shared__ double cam[5];
  __shared__ float tcw[12];
  if (threadIdx.x < 5) cam[threadIdx.x] = D.cam[threadIdx.x];
  if (threadIdx.x < 12) tcw[threadIdx.x] = D.tcw[threadIdx.x];
  if (threadIdx.x == 0) work.positive = 0;
  __syncthreads();
  P.fx = cam[0], P.fy = cam[1], P.cx = cam[2], P.cy = cam[3], P.bf = cam[4];
  P.tcw = tcw;
  LmDevGroup g;
  g.red = red;
  po_optimize(g, P, work, reinterpret_cast<PoOut*>(res + D.o_out),
              reinterpret_cast<uint64_t*>(res + D.o_mask));
}

// ------------------------------------------------------------------------------------------
// host

struct orbfe_poseopt : OrbfeDev {
  int S = 0, C = 0;
  OrbfeStage in, res;  // inputs (one upload), results (one copy back); sized by po_plan_bounds
};

extern "C" int orbfe_poseopt_create(int device, int max_problems, int max_obs, orbfe_poseopt** out) {
  if (!out) return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_poseopt_create: bad argument");
  *out = nullptr;
  if (max_problems < 1 || max_problems > ORBFE_POSEOPT_MAX_PROBLEMS || max_obs < 1 || max_obs > ORBFE_POSEOPT_MAX_OBS)
    return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_poseopt_create: max_problems in 1..64, max_obs in 1..4096");
  orbfe_poseopt* h = new orbfe_poseopt();
  h->S = max_problems;
  h->C = max_obs;
  if (device < 0) {
    *out = h;
    return ORBFE_OK;
  }
  const int st = orbfe_dev_open(h, device, "orbfe_poseopt_create");
  if (st != ORBFE_OK) {
    orbfe_poseopt_destroy(h);
    return st;
  }
  size_t in_bytes, res_bytes;
  po_plan_bounds(h->S, h->C, &in_bytes, &res_bytes);
  ORBFE_CREATE_HIP(h, orbfe_poseopt_destroy, orbfe_stage_alloc(&h->in, in_bytes, true));
  ORBFE_CREATE_HIP(h, orbfe_poseopt_destroy, orbfe_stage_alloc(&h->res, res_bytes, true));
  *out = h;
  return ORBFE_OK;
}

extern "C" int orbfe_poseopt_destroy(orbfe_poseopt* h) {
  if (!h) return ORBFE_OK;
  if (orbfe_dev_close(h)) {
    orbfe_stage_free(&h->in);
    orbfe_stage_free(&h->res);
  }
  delete h;
  return ORBFE_OK;
}

static int po_check_problem(const orbfe_poseopt* h, const orbfe_poseopt_problem_t* p, const orbfe_poseopt_result_t* r) {
  if (p->n < 0 || r->mask_words < 0) return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_poseopt_batch: bad n or mask_words");
  if (p->n > h->C) return orbfe_set_error(ORBFE_ERR_CAPACITY, "orbfe_poseopt_batch: n above the handle's max_obs");
  if (p->n > 0 && (!p->valid || !p->xw || !p->kp_un || !p->u_right || !p->inv_sigma2))
    return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_poseopt_batch: null observation array");
  if (r->outlier_mask && r->mask_words < (p->n + 63) / 64)
    return orbfe_set_error(ORBFE_ERR_CAPACITY, "orbfe_poseopt_batch: mask_words below ceil(n / 64)");
  return ORBFE_OK;
}

extern "C" int orbfe_poseopt_batch(orbfe_poseopt* h, const orbfe_poseopt_problem_t* problems, int n_problems,
                                   orbfe_poseopt_result_t* results) {
  if (!h || !problems || !results || n_problems < 1)
    return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_poseopt_batch: bad argument");
  if (n_problems > h->S)
    return orbfe_set_error(ORBFE_ERR_CAPACITY, "orbfe_poseopt_batch: more problems than the handle's max_problems");
  for (int i = 0; i < n_problems; i++) {
    const int st = po_check_problem(h, &problems[i], &results[i]);
    if (st != ORBFE_OK) return st;
  }
  if (h->device < 0) return orbfe_set_error(ORBFE_ERR_STATE, "pose optimizer is host-only (device < 0)");
  OrbfeStage &in = h->in, &res = h->res;
  in.off = res.off = 0;
  PoDev* dev;
  in.take<PoDev>((size_t)n_problems, &dev);
  for (int i = 0; i < n_problems; i++) {
    const orbfe_poseopt_problem_t& p = problems[i];
    const size_t n = (size_t)p.n;
    PoDev d;
    memset(&d, 0, sizeof(d));
    d.n = p.n;
    for (int k = 0; k < 4; k++) d.cam[k] = (double)p.k[k];  // e->fx = pFrame->fx ...: float widened to double
    d.cam[4] = (double)p.bf;
    memcpy(d.tcw, p.tcw, sizeof(d.tcw));
    po_layout(in, res, n, d);
    if (in.off > in.cap || res.off > res.cap)  // cannot happen within the bounds
      return orbfe_set_error(ORBFE_ERR_CAPACITY, "orbfe_poseopt_batch: staging plan exceeds the handle's buffers");
    if (n > 0) {
      memcpy(in.h + d.in_valid, p.valid, n);
      memcpy(in.h + d.in_xw, p.xw, 12 * n);
      memcpy(in.h + d.in_kp, p.kp_un, 8 * n);
      memcpy(in.h + d.in_ur, p.u_right, 4 * n);
      memcpy(in.h + d.in_is2, p.inv_sigma2, 4 * n);
    }
    dev[i] = d;
  }
  ORBFE_HIP_CHECK(hipSetDevice(h->device));
  int st;
  if ((st = orbfe_stage_upload(&in, h->stream)) != ORBFE_OK) return st;
  const uint8_t* din = in.d;
  uint8_t* dres = res.d;
  ORBFE_LAUNCH("k_poseopt", k_poseopt, dim3(n_problems), dim3(PO_LANES), 0, h->stream, din, dres);
  if ((st = orbfe_stage_download(&res, h->stream)) != ORBFE_OK) return st;
  for (int i = 0; i < n_problems; i++) {
    const PoDev& d = dev[i];
    orbfe_poseopt_result_t& r = results[i];
    const PoOut* o = reinterpret_cast<const PoOut*>(res.h + d.o_out);
    memcpy(r.tcw, o->tcw, sizeof(r.tcw));
    memcpy(r.pose_q_t, o->pose, sizeof(r.pose_q_t));
    r.n_initial = o->n_initial;
    r.n_bad = o->n_bad;
    r.n_inliers = o->n_inliers;
    r.rounds_run = o->rounds_run;
    r.flags = o->flags;
    memcpy(r.rounds, o->rounds, sizeof(r.rounds));
    if (r.outlier_mask) orbfe_unpack_masks(r.outlier_mask, r.mask_words, res.h + d.o_mask, (d.n + 63) / 64, 1);
  }
  return ORBFE_OK;
}
