// orbfe_optsim3.hip -- Optimizer::OptimizeSim3 on the GPU (include/orbfe_optsim3.h): a batch of 7-DoF
// Levenberg-Marquardt problems, one wavefront each.
//
//   k_optsim3  one block of 64 lanes per problem. Per linearisation lanes 0..14 build the estimate,
//              its 14 perturbed neighbours oplus(+-1e-9 e_d) and all their inverses into LDS (30 x 8
//              doubles); every lane then evaluates its correspondences' two edges at the 15 states
//              for the numeric Jacobians. The sums of H, b and chi2 cross the lanes by the fixed
//              shuffle tree, lane 0 factors the 7x7 system in LDS, and both rounds with their
//              classifications run inside the one launch
//
// One call stages every problem in one pinned buffer (one H2D copy), launches once on the handle's
// stream and takes every result down in one D2H copy. All offsets are formed on the host from counts
// it has checked against the handle's bounds; the kernel indexes the arrays only with i < n from its
// strided loops. The removal flags of a lane's correspondences are the bits of one 64-bit register
// (max_obs <= 64 * 64) and the stale errors are recomputed from the last evaluated estimate, so the
// kernel needs no per-edge workspace.
//
// Resources (-Rpass-analysis=kernel-resource-usage, gfx950): 256 VGPRs, 106 SGPRs (36 spilled to vector
// lanes), 0 bytes of scratch, no VGPR spill, 10,448 bytes of LDS per block. An edge's Jacobian goes through
// the lane's column of OsWork::J in LDS with the loop over the 7 dimensions kept rolled; unrolled, the
// table's loads were hoisted out of the correspondence loop and the kernel spilled.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>

#include "../../include/orbfe_optsim3.h"
#include "orbfe_device.h"
#include "orbfe_ktimer.h"
#include "orbfe_lm_device.h"
#include "orbfe_optsim3_core.h"
#include "orbfe_stage.h"

static_assert(ORBFE_OPTSIM3_MAX_OBS <= PO_LANES * 64, "a lane's removal flags are one 64-bit word");
static_assert(sizeof(PoRound) == sizeof(orbfe_poseopt_round_t), "trace layout");

__global__ __launch_bounds__(PO_LANES) void k_optsim3(const uint8_t* __restrict__ in, uint8_t* __restrict__ res) {
  const OsDev& D = reinterpret_cast<const OsDev*>(in)[blockIdx.x];
  __shared__ OsWork work;
  __shared__ double red[OS_ACC];
  // the cameras and the start go through LDS for the same reason as the sums (LmDevGroup::reduce)
  __shared__ double cam[9];
  __shared__ float start[13];
  __shared__ float kf2[12];
  if (threadIdx.x < 9) cam[threadIdx.x] = D.cam[threadIdx.x];
  if (threadIdx.x < 13) start[threadIdx.x] = D.start[threadIdx.x];
  if (threadIdx.x < 12) kf2[threadIdx.x] = D.kf2[threadIdx.x];
  if (threadIdx.x == 0) work.positive = 0;
  __syncthreads();
  OsProblem P;
  P.n = D.n;
  P.fix_scale = D.fix_scale;
  P.has_kf2 = D.has_kf2;
  P.valid = in + D.in_valid;
  P.p3d1c = reinterpret_cast<const float*>(in + D.in_p1);
  P.p3d2c = reinterpret_cast<const float*>(in + D.in_p2);
  P.kp1 = reinterpret_cast<const float*>(in + D.in_kp1);
  P.kp2 = reinterpret_cast<const float*>(in + D.in_kp2);
  P.is1 = reinterpret_cast<const float*>(in + D.in_is1);
  P.is2 = reinterpret_cast<const float*>(in + D.in_is2);
#pragma unroll
  for (int k = 0; k < 4; k++) P.k1[k] = cam[k], P.k2[k] = cam[4 + k];
  P.th2 = cam[8];
  P.start = start;
  P.kf2 = kf2;
  LmDevGroup g;
  g.red = red;
  os_optimize(g, P, work, reinterpret_cast<OsOut*>(res + D.o_out), reinterpret_cast<uint64_t*>(res + D.o_mask));
}

// ------------------------------------------------------------------------------------------
// host

struct orbfe_optsim3 : OrbfeDev {
  int S = 0, C = 0;
  OrbfeStage in, res;  // inputs (one upload), results (one copy back); sized by os_plan_bounds
};

extern "C" int orbfe_optsim3_create(int device, int max_problems, int max_obs, orbfe_optsim3** out) {
  if (!out) return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_optsim3_create: bad argument");
  *out = nullptr;
  if (max_problems < 1 || max_problems > ORBFE_OPTSIM3_MAX_PROBLEMS || max_obs < 1 || max_obs > ORBFE_OPTSIM3_MAX_OBS)
    return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_optsim3_create: max_problems in 1..64, max_obs in 1..4096");
  orbfe_optsim3* h = new orbfe_optsim3();
  h->S = max_problems;
  h->C = max_obs;
  if (device < 0) {
    *out = h;
    return ORBFE_OK;
  }
  const int st = orbfe_dev_open(h, device, "orbfe_optsim3_create");
  if (st != ORBFE_OK) {
    orbfe_optsim3_destroy(h);
    return st;
  }
  size_t in_bytes, res_bytes;
  os_plan_bounds(h->S, h->C, &in_bytes, &res_bytes);
  ORBFE_CREATE_HIP(h, orbfe_optsim3_destroy, orbfe_stage_alloc(&h->in, in_bytes, true));
  ORBFE_CREATE_HIP(h, orbfe_optsim3_destroy, orbfe_stage_alloc(&h->res, res_bytes, true));
  *out = h;
  return ORBFE_OK;
}

extern "C" int orbfe_optsim3_destroy(orbfe_optsim3* h) {
  if (!h) return ORBFE_OK;
  if (orbfe_dev_close(h)) {
    orbfe_stage_free(&h->in);
    orbfe_stage_free(&h->res);
  }
  delete h;
  return ORBFE_OK;
}

static int os_check_problem(const orbfe_optsim3* h, const orbfe_optsim3_problem_t* p, const orbfe_optsim3_result_t* r) {
  if (p->n < 0 || r->mask_words < 0) return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_optsim3_batch: bad n or mask_words");
  if (p->n > h->C) return orbfe_set_error(ORBFE_ERR_CAPACITY, "orbfe_optsim3_batch: n above the handle's max_obs");
  if (p->n > 0 && (!p->valid || !p->p3d1c || !p->p3d2c || !p->kp_un1 || !p->kp_un2 || !p->inv_sigma2_1 || !p->inv_sigma2_2))
    return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_optsim3_batch: null correspondence array");
  if (r->removed_mask && r->mask_words < (p->n + 63) / 64)
    return orbfe_set_error(ORBFE_ERR_CAPACITY, "orbfe_optsim3_batch: mask_words below ceil(n / 64)");
  return ORBFE_OK;
}

extern "C" int orbfe_optsim3_batch(orbfe_optsim3* h, const orbfe_optsim3_problem_t* problems, int n_problems,
                                   orbfe_optsim3_result_t* results) {
  if (!h || !problems || !results || n_problems < 1)
    return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_optsim3_batch: bad argument");
  if (n_problems > h->S)
    return orbfe_set_error(ORBFE_ERR_CAPACITY, "orbfe_optsim3_batch: more problems than the handle's max_problems");
  for (int i = 0; i < n_problems; i++) {
    const int st = os_check_problem(h, &problems[i], &results[i]);
    if (st != ORBFE_OK) return st;
  }
  if (h->device < 0) return orbfe_set_error(ORBFE_ERR_STATE, "Sim3 optimizer is host-only (device < 0)");
  OrbfeStage &in = h->in, &res = h->res;
  in.off = res.off = 0;
  OsDev* dev;
  in.take<OsDev>((size_t)n_problems, &dev);
  for (int i = 0; i < n_problems; i++) {
    const orbfe_optsim3_problem_t& p = problems[i];
    const size_t n = (size_t)p.n;
    OsDev d;
    memset(&d, 0, sizeof(d));
    d.n = p.n;
    d.fix_scale = p.fix_scale ? 1 : 0;
    d.has_kf2 = p.has_kf2 ? 1 : 0;
    for (int k = 0; k < 4; k++) d.cam[k] = (double)p.k1[k], d.cam[4 + k] = (double)p.k2[k];  // K.at<float>: widened
    d.cam[8] = (double)p.th2;
    memcpy(d.start, p.r12, sizeof(p.r12));
    memcpy(d.start + 9, p.t12, sizeof(p.t12));
    d.start[12] = p.s12;
    if (d.has_kf2) {
      memcpy(d.kf2, p.r2w, sizeof(p.r2w));
      memcpy(d.kf2 + 9, p.t2w, sizeof(p.t2w));
    }
    os_layout(in, res, n, d);
    if (in.off > in.cap || res.off > res.cap)  // cannot happen within the bounds
      return orbfe_set_error(ORBFE_ERR_CAPACITY, "orbfe_optsim3_batch: staging plan exceeds the handle's buffers");
    if (n > 0) {
      memcpy(in.h + d.in_valid, p.valid, n);
      memcpy(in.h + d.in_p1, p.p3d1c, 12 * n);
      memcpy(in.h + d.in_p2, p.p3d2c, 12 * n);
      memcpy(in.h + d.in_kp1, p.kp_un1, 8 * n);
      memcpy(in.h + d.in_kp2, p.kp_un2, 8 * n);
      memcpy(in.h + d.in_is1, p.inv_sigma2_1, 4 * n);
      memcpy(in.h + d.in_is2, p.inv_sigma2_2, 4 * n);
    }
    dev[i] = d;
  }
  ORBFE_HIP_CHECK(hipSetDevice(h->device));
  int st;
  if ((st = orbfe_stage_upload(&in, h->stream)) != ORBFE_OK) return st;
  const uint8_t* din = in.d;
  uint8_t* dres = res.d;
  ORBFE_LAUNCH("k_optsim3", k_optsim3, dim3(n_problems), dim3(PO_LANES), 0, h->stream, din, dres);
  if ((st = orbfe_stage_download(&res, h->stream)) != ORBFE_OK) return st;
  for (int i = 0; i < n_problems; i++) {
    const OsDev& d = dev[i];
    orbfe_optsim3_result_t& r = results[i];
    const OsOut* o = reinterpret_cast<const OsOut*>(res.h + d.o_out);
    memcpy(r.sim3_q_t_s, o->sim3, sizeof(r.sim3_q_t_s));
    memcpy(r.s12_rt, o->s12_rt, sizeof(r.s12_rt));
    memcpy(r.scw, o->scw, sizeof(r.scw));
    r.n_correspondences = o->n_correspondences;
    r.n_bad = o->n_bad;
    r.n_inliers = o->n_inliers;
    r.rounds_run = o->rounds_run;
    r.flags = o->flags;
    memcpy(r.rounds, o->rounds, sizeof(r.rounds));
    if (r.removed_mask) orbfe_unpack_masks(r.removed_mask, r.mask_words, res.h + d.o_mask, (d.n + 63) / 64, 1);
  }
  return ORBFE_OK;
}
