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

static_assert(LM_FLAG_LARGE_STEP == ORBFE_POSEOPT_FLAG_LARGE_STEP && LM_FLAG_NONFINITE == ORBFE_POSEOPT_FLAG_NONFINITE,
              "flag values");
static_assert(LM_STOP_ALL == ORBFE_POSEOPT_STOP_ALL && LM_STOP_TERMINATE == ORBFE_POSEOPT_STOP_TERMINATE &&
                  LM_STOP_NBAD == ORBFE_POSEOPT_STOP_NBAD && LM_STOP_NO_EDGE == ORBFE_POSEOPT_STOP_NO_EDGE,
              "stop codes");
static_assert(ORBFE_POSEOPT_MAX_OBS <= PO_LANES * 64, "a lane's outlier flags are one 64-bit word");
static_assert(sizeof(PoRound) == sizeof(orbfe_poseopt_round_t), "trace layout");

// One problem as the kernel sees it. in_* are byte offsets into the upload buffer, o_* into the result
// buffer.
struct PoDev {
  int n, pad;
  double cam[5];  // fx, fy, cx, cy, bf: float widened to double
  float tcw[12];
  unsigned long long in_valid, in_xw, in_kp, in_ur, in_is2, o_out, o_mask;
};

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

struct orbfe_poseopt {
  int device = -1;
  int S = 0, C = 0;
  hipStream_t stream = nullptr;
  uint8_t *d_in = nullptr, *h_in = nullptr, *d_res = nullptr, *h_res = nullptr;
  size_t in_bytes = 0, res_bytes = 0;
};

static size_t po_al(size_t b) { return (b + 255) & ~(size_t)255; }
static size_t po_in_bytes(size_t n) { return po_al(n) + po_al(12 * n) + po_al(8 * n) + 2 * po_al(4 * n); }
static size_t po_res_bytes(size_t n) { return po_al(sizeof(PoOut)) + po_al(8 * ((n + 63) / 64)); }

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
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device >= ndev) {
    delete h;
    return orbfe_set_error(ORBFE_ERR_HIP, "orbfe_poseopt_create: no such HIP device");
  }
  h->device = device;
  h->in_bytes = po_al(sizeof(PoDev) * (size_t)h->S) + (size_t)h->S * po_in_bytes(h->C);
  h->res_bytes = (size_t)h->S * po_res_bytes(h->C);
  auto fail = [&](hipError_t e, const char* what) {
    const int st = orbfe_set_hip_error(e, what);
    orbfe_poseopt_destroy(h);
    return st;
  };
#define PO_TRY(expr)                              \
  do {                                            \
    hipError_t _e = (expr);                       \
    if (_e != hipSuccess) return fail(_e, #expr); \
  } while (0)
  PO_TRY(hipSetDevice(device));
  PO_TRY(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  PO_TRY(hipMalloc(&h->d_in, h->in_bytes));
  PO_TRY(hipMalloc(&h->d_res, h->res_bytes));
  PO_TRY(hipHostMalloc(&h->h_in, h->in_bytes, hipHostMallocDefault));
  PO_TRY(hipHostMalloc(&h->h_res, h->res_bytes, hipHostMallocDefault));
#undef PO_TRY
  *out = h;
  return ORBFE_OK;
}

extern "C" int orbfe_poseopt_destroy(orbfe_poseopt* h) {
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
  PoDev* dev = reinterpret_cast<PoDev*>(h->h_in);
  size_t in_off = po_al(sizeof(PoDev) * (size_t)n_problems), res_off = 0;
  for (int i = 0; i < n_problems; i++) {
    const orbfe_poseopt_problem_t& p = problems[i];
    const size_t n = (size_t)p.n;
    PoDev d;
    memset(&d, 0, sizeof(d));
    d.n = p.n;
    for (int k = 0; k < 4; k++) d.cam[k] = (double)p.k[k];  // e->fx = pFrame->fx ...: float widened to double
    d.cam[4] = (double)p.bf;
    memcpy(d.tcw, p.tcw, sizeof(d.tcw));
    auto take_in = [&](size_t bytes) {
      const size_t o = in_off;
      in_off += po_al(bytes);
      return o;
    };
    d.in_valid = take_in(n);
    d.in_xw = take_in(12 * n);
    d.in_kp = take_in(8 * n);
    d.in_ur = take_in(4 * n);
    d.in_is2 = take_in(4 * n);
    d.o_out = res_off;
    res_off += po_al(sizeof(PoOut));
    d.o_mask = res_off;
    res_off += po_al(8 * ((n + 63) / 64));
    if (in_off > h->in_bytes || res_off > h->res_bytes)  // cannot happen within the bounds
      return orbfe_set_error(ORBFE_ERR_CAPACITY, "orbfe_poseopt_batch: staging plan exceeds the handle's buffers");
    if (n > 0) {
      memcpy(h->h_in + d.in_valid, p.valid, n);
      memcpy(h->h_in + d.in_xw, p.xw, 12 * n);
      memcpy(h->h_in + d.in_kp, p.kp_un, 8 * n);
      memcpy(h->h_in + d.in_ur, p.u_right, 4 * n);
      memcpy(h->h_in + d.in_is2, p.inv_sigma2, 4 * n);
    }
    dev[i] = d;
  }
  ORBFE_HIP_CHECK(hipSetDevice(h->device));
  ORBFE_HIP_CHECK(hipMemcpyAsync(h->d_in, h->h_in, in_off, hipMemcpyHostToDevice, h->stream));
  const uint8_t* din = h->d_in;
  uint8_t* dres = h->d_res;
  ORBFE_LAUNCH("k_poseopt", k_poseopt, dim3(n_problems), dim3(PO_LANES), 0, h->stream, din, dres);
  ORBFE_HIP_CHECK(hipGetLastError());
  ORBFE_HIP_CHECK(hipMemcpyAsync(h->h_res, h->d_res, res_off, hipMemcpyDeviceToHost, h->stream));
  ORBFE_HIP_CHECK(hipStreamSynchronize(h->stream));
  for (int i = 0; i < n_problems; i++) {
    const PoDev& d = dev[i];
    orbfe_poseopt_result_t& r = results[i];
    const PoOut* o = reinterpret_cast<const PoOut*>(h->h_res + d.o_out);
    memcpy(r.tcw, o->tcw, sizeof(r.tcw));
    memcpy(r.pose_q_t, o->pose, sizeof(r.pose_q_t));
    r.n_initial = o->n_initial;
    r.n_bad = o->n_bad;
    r.n_inliers = o->n_inliers;
    r.rounds_run = o->rounds_run;
    r.flags = o->flags;
    memcpy(r.rounds, o->rounds, sizeof(r.rounds));
    if (r.outlier_mask) {
      const int words = (d.n + 63) / 64;
      memcpy(r.outlier_mask, h->h_res + d.o_mask, 8 * (size_t)words);
      for (int w = words; w < r.mask_words; w++) r.outlier_mask[w] = 0;
    }
  }
  return ORBFE_OK;
}
