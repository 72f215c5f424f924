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

static_assert(ORBFE_OPTSIM3_MAX_OBS <= PO_LANES * 64, "a lane's removal flags are one 64-bit word");
static_assert(sizeof(PoRound) == sizeof(orbfe_poseopt_round_t), "trace layout");

// One problem as the kernel sees it. in_* are byte offsets into the upload buffer, o_* into the result
// buffer.
struct OsDev {
  int n, fix_scale, has_kf2, pad;
  double cam[9];    // k1, k2 (fx, fy, cx, cy: float widened to double), th2
  float start[13];  // r12, t12, s12
  float kf2[12];    // r2w, t2w
  float pad2;
  unsigned long long in_valid, in_p1, in_p2, in_kp1, in_kp2, in_is1, in_is2, o_out, o_mask;
};

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

struct orbfe_optsim3 {
  int device = -1;
  int S = 0, C = 0;
  hipStream_t stream = nullptr;
  uint8_t *d_in = nullptr, *h_in = nullptr, *d_res = nullptr, *h_res = nullptr;
  size_t in_bytes = 0, res_bytes = 0;
};

static size_t os_al(size_t b) { return (b + 255) & ~(size_t)255; }
static size_t os_in_bytes(size_t n) { return os_al(n) + 2 * os_al(12 * n) + 2 * os_al(8 * n) + 2 * os_al(4 * n); }
static size_t os_res_bytes(size_t n) { return os_al(sizeof(OsOut)) + os_al(8 * ((n + 63) / 64)); }

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
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device >= ndev) {
    delete h;
    return orbfe_set_error(ORBFE_ERR_HIP, "orbfe_optsim3_create: no such HIP device");
  }
  h->device = device;
  h->in_bytes = os_al(sizeof(OsDev) * (size_t)h->S) + (size_t)h->S * os_in_bytes(h->C);
  h->res_bytes = (size_t)h->S * os_res_bytes(h->C);
  auto fail = [&](hipError_t e, const char* what) {
    const int st = orbfe_set_hip_error(e, what);
    orbfe_optsim3_destroy(h);
    return st;
  };
#define OS_TRY(expr)                              \
  do {                                            \
    hipError_t _e = (expr);                       \
    if (_e != hipSuccess) return fail(_e, #expr); \
  } while (0)
  OS_TRY(hipSetDevice(device));
  OS_TRY(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  OS_TRY(hipMalloc(&h->d_in, h->in_bytes));
  OS_TRY(hipMalloc(&h->d_res, h->res_bytes));
  OS_TRY(hipHostMalloc(&h->h_in, h->in_bytes, hipHostMallocDefault));
  OS_TRY(hipHostMalloc(&h->h_res, h->res_bytes, hipHostMallocDefault));
#undef OS_TRY
  *out = h;
  return ORBFE_OK;
}

extern "C" int orbfe_optsim3_destroy(orbfe_optsim3* h) {
  if (!h) return ORBFE_OK;
  if (h->device >= 0) {
    hipSetDevice(h->device);
    if (h->stream) hipStreamSynchronize(h->stream);
    hipFree(h->d_in);
    hipFree(h->d_res);
    if (h->h_in) hipHostFree(h->h_in);
    if (h->h_res) hipHostFree(h->h_res);
    if (h->stream) hipStreamDestroy(h->stream);
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
  OsDev* dev = reinterpret_cast<OsDev*>(h->h_in);
  size_t in_off = os_al(sizeof(OsDev) * (size_t)n_problems), res_off = 0;
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
    auto take_in = [&](size_t bytes) {
      const size_t o = in_off;
      in_off += os_al(bytes);
      return o;
    };
    d.in_valid = take_in(n);
    d.in_p1 = take_in(12 * n);
    d.in_p2 = take_in(12 * n);
    d.in_kp1 = take_in(8 * n);
    d.in_kp2 = take_in(8 * n);
    d.in_is1 = take_in(4 * n);
    d.in_is2 = take_in(4 * n);
    d.o_out = res_off;
    res_off += os_al(sizeof(OsOut));
    d.o_mask = res_off;
    res_off += os_al(8 * ((n + 63) / 64));
    if (in_off > h->in_bytes || res_off > h->res_bytes)  // cannot happen within the bounds
      return orbfe_set_error(ORBFE_ERR_CAPACITY, "orbfe_optsim3_batch: staging plan exceeds the handle's buffers");
    if (n > 0) {
      memcpy(h->h_in + d.in_valid, p.valid, n);
      memcpy(h->h_in + d.in_p1, p.p3d1c, 12 * n);
      memcpy(h->h_in + d.in_p2, p.p3d2c, 12 * n);
      memcpy(h->h_in + d.in_kp1, p.kp_un1, 8 * n);
      memcpy(h->h_in + d.in_kp2, p.kp_un2, 8 * n);
      memcpy(h->h_in + d.in_is1, p.inv_sigma2_1, 4 * n);
      memcpy(h->h_in + d.in_is2, p.inv_sigma2_2, 4 * n);
    }
    dev[i] = d;
  }
  ORBFE_HIP_CHECK(hipSetDevice(h->device));
  ORBFE_HIP_CHECK(hipMemcpyAsync(h->d_in, h->h_in, in_off, hipMemcpyHostToDevice, h->stream));
  const uint8_t* din = h->d_in;
  uint8_t* dres = h->d_res;
  ORBFE_LAUNCH("k_optsim3", k_optsim3, dim3(n_problems), dim3(PO_LANES), 0, h->stream, din, dres);
  ORBFE_HIP_CHECK(hipGetLastError());
  ORBFE_HIP_CHECK(hipMemcpyAsync(h->h_res, h->d_res, res_off, hipMemcpyDeviceToHost, h->stream));
  ORBFE_HIP_CHECK(hipStreamSynchronize(h->stream));
  for (int i = 0; i < n_problems; i++) {
    const OsDev& d = dev[i];
    orbfe_optsim3_result_t& r = results[i];
    const OsOut* o = reinterpret_cast<const OsOut*>(h->h_res + d.o_out);
    memcpy(r.sim3_q_t_s, o->sim3, sizeof(r.sim3_q_t_s));
    memcpy(r.s12_rt, o->s12_rt, sizeof(r.s12_rt));
    memcpy(r.scw, o->scw, sizeof(r.scw));
    r.n_correspondences = o->n_correspondences;
    r.n_bad = o->n_bad;
    r.n_inliers = o->n_inliers;
    r.rounds_run = o->rounds_run;
    r.flags = o->flags;
    memcpy(r.rounds, o->rounds, sizeof(r.rounds));
    if (r.removed_mask) {
      const int words = (d.n + 63) / 64;
      memcpy(r.removed_mask, h->h_res + d.o_mask, 8 * (size_t)words);
      for (int w = words; w < r.mask_words; w++) r.removed_mask[w] = 0;
    }
  }
  return ORBFE_OK;
}
