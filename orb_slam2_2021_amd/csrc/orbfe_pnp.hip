// orbfe_pnp.hip -- PnPsolver on the GPU (include/orbfe_pnp.h): batched EPnP RANSAC over the
// correspondences of several relocalisation candidates.
//
//   k_pnp_hypotheses  16 lanes per hypothesis, 4 per wavefront: swap-remove selection + EPnP, the
//                     working set (PnpWork) in LDS
//   k_pnp_inliers     one wavefront per pose: CheckInliers over all correspondences (hypotheses, then
//                     the refined poses)
//   k_pnp_records     one thread per solver: the prefix-record scan over the inlier counts
//   k_pnp_refine      one wavefront per record: gather of the record's inliers + EPnP over them
//   k_pnp_select      one thread per solver: find() replayed
//
// One call stages every solver's inputs in one pinned buffer (one H2D copy), launches the kernels on
// the handle's stream and takes every result down in one D2H copy. All offsets into the buffers are
// formed on the host from counts it has checked against the handle's bounds; every index a kernel
// forms comes from a bounded loop, a host-checked draw or an inlier bit below n.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/orbfe_pnp.h"
#include "orbfe_device.h"
#include "orbfe_ktimer.h"
#include "orbfe_match_internal.h"
#include "orbfe_pnp_core.h"
#include "orbfe_stage.h"

static_assert(PNP_FLAG_SVD_NULL == ORBFE_PNP_FLAG_SVD_NULL && PNP_FLAG_QR_SINGULAR == ORBFE_PNP_FLAG_QR_SINGULAR,
              "flag values");
static_assert(PNP_R == ORBFE_PNP_MAX_RECORDS, "records per solver");

#define PNP_HYP_PER_BLOCK 4
#define PNP_INL_THREADS 256
#define PNP_INL_WAVES (PNP_INL_THREADS / 64)

template <int W>
struct PnpDevGroup {
  static constexpr int width = W;
  __device__ int lane() const { return threadIdx.x & (W - 1); }
  __device__ void sync() const { __syncthreads(); }  // the block is one wavefront
  __device__ bool all(bool b) const { return __all(b); }
};

__device__ __forceinline__ void pnp_store_pose(const double* R, const double* t, int N, unsigned flags, double* oR,
                                               double* ot, float* otcw, int32_t* oN, uint32_t* oflags) {
  for (int i = 0; i < 9; i++) oR[i] = R[i];
  for (int i = 0; i < 3; i++) ot[i] = t[i];
  for (int i = 0; i < 3; i++) {  // Rcw / tcw .convertTo(CV_32F) (:228-234)
    for (int j = 0; j < 3; j++) otcw[4 * i + j] = (float)R[3 * i + j];
    otcw[4 * i + 3] = (float)t[i];
  }
  *oN = N;
  *oflags = flags;
}

__global__ __launch_bounds__(64) void k_pnp_hypotheses(const uint8_t* __restrict__ in, uint8_t* __restrict__ res) {
  const PnpDev& P = reinterpret_cast<const PnpDev*>(in)[blockIdx.y];
  if ((int)blockIdx.x * PNP_HYP_PER_BLOCK >= P.n_eval) return;  // block-uniform
  __shared__ PnpWork work[PNP_HYP_PER_BLOCK];
  __shared__ double pts[PNP_HYP_PER_BLOCK][48];  // pws 12, us 8, alphas 16, pcs 12
  __shared__ double pose[PNP_HYP_PER_BLOCK][12];
  __shared__ int chosen[PNP_HYP_PER_BLOCK];
  __shared__ unsigned flg[PNP_HYP_PER_BLOCK];
  const int grp = threadIdx.x >> 4, lane = threadIdx.x & 15;
  const int k0 = blockIdx.x * PNP_HYP_PER_BLOCK + grp;
  const bool active = k0 < P.n_eval;
  const int k = active ? k0 : P.n_eval - 1;  // a group past the end repeats the last hypothesis and stores nothing
  double* pws = pts[grp];
  double* us = pws + 12;
  double* alphas = us + 8;
  double* pcs = alphas + 16;
  if (lane == 0) {
    const int32_t* draw = reinterpret_cast<const int32_t*>(in + P.in_rand) + 4 * (size_t)k;
    const int d[4] = {draw[0], draw[1], draw[2], draw[3]};  // checked by the host: 0 <= d[i] <= n-1-i
    int idx[4];
    pnp_select4(P.n, d, idx);
    const float* p3 = reinterpret_cast<const float*>(in + P.in_p3d);
    const float* p2 = reinterpret_cast<const float*>(in + P.in_p2d);
    for (int c = 0; c < 4; c++) {  // add_correspondence (:373-383): float -> double
      const size_t i = (size_t)idx[c];
      pws[3 * c] = p3[3 * i], pws[3 * c + 1] = p3[3 * i + 1], pws[3 * c + 2] = p3[3 * i + 2];
      us[2 * c] = p2[2 * i], us[2 * c + 1] = p2[2 * i + 1];
    }
  }
  __syncthreads();
  pnp_compute_pose(PnpDevGroup<16>(), work[grp], 4, pws, us, alphas, pcs, P.K, pose[grp], pose[grp] + 9, &chosen[grp],
                   &flg[grp]);
  if (lane == 0 && active)
    pnp_store_pose(pose[grp], pose[grp] + 9, chosen[grp], flg[grp],
                   reinterpret_cast<double*>(res + P.o_r) + 9 * (size_t)k,
                   reinterpret_cast<double*>(res + P.o_t) + 3 * (size_t)k,
                   reinterpret_cast<float*>(res + P.o_tcw) + 12 * (size_t)k,
                   reinterpret_cast<int32_t*>(res + P.o_N) + k, reinterpret_cast<uint32_t*>(res + P.o_flags) + k);
}

// refined == 0: pose k of the evaluated hypotheses; refined == 1: pose of record slot k
__global__ __launch_bounds__(PNP_INL_THREADS) void k_pnp_inliers(const uint8_t* __restrict__ in,
                                                                 uint8_t* __restrict__ res, int refined) {
  const PnpDev& P = reinterpret_cast<const PnpDev*>(in)[blockIdx.y];
  const int lane = threadIdx.x & 63;
  const int k = blockIdx.x * PNP_INL_WAVES + (threadIdx.x >> 6);  // wave-uniform
  const int limit = refined ? reinterpret_cast<const int32_t*>(res + P.o_sel)[5] : P.n_eval;  // n_records <= PNP_R
  if (k >= limit) return;
  const double* gR = reinterpret_cast<const double*>(res + (refined ? P.o_rr : P.o_r)) + 9 * (size_t)k;
  const double* gt = reinterpret_cast<const double*>(res + (refined ? P.o_rt : P.o_t)) + 3 * (size_t)k;
  double R[9], t[3], K[4];
  for (int i = 0; i < 9; i++) R[i] = gR[i];
  for (int i = 0; i < 3; i++) t[i] = gt[i];
  for (int i = 0; i < 4; i++) K[i] = P.K[i];
  const float* p3 = reinterpret_cast<const float*>(in + P.in_p3d);
  const float* p2 = reinterpret_cast<const float*>(in + P.in_p2d);
  const float* mx = reinterpret_cast<const float*>(in + P.in_max);
  unsigned long long* mask =
      reinterpret_cast<unsigned long long*>(res + (refined ? P.o_rmask : P.o_mask)) + (size_t)P.words * k;
  const int n = P.n;
  int count = 0;
  for (int c0 = 0; c0 < n; c0 += 64) {  // c0 / 64 < words = ceil(n / 64)
    const int i = c0 + lane;
    bool inl = false;
    if (i < n)
      inl = pnp_is_inlier(R, t, K, p3[3 * (size_t)i], p3[3 * (size_t)i + 1], p3[3 * (size_t)i + 2], p2[2 * (size_t)i],
                          p2[2 * (size_t)i + 1], mx[i]);
    const unsigned long long word = __ballot(inl);
    count += __popcll(word);
    if (lane == 0) mask[c0 >> 6] = word;
  }
  if (lane == 0) reinterpret_cast<int32_t*>(res + (refined ? P.o_rcnt : P.o_cnt))[k] = count;
}

// The records of a solver: hypothesis k with count >= mRansacMinInliers and above every earlier one
// (:220-226). slot[k] = its position in the record list or -1; past PNP_R records the scan stops.
__global__ __launch_bounds__(64) void k_pnp_records(const uint8_t* __restrict__ in, uint8_t* __restrict__ res,
                                                    int n_solvers) {
  const int sidx = threadIdx.x;
  if (sidx >= n_solvers) return;
  const PnpDev& P = reinterpret_cast<const PnpDev*>(in)[sidx];
  const int32_t* cnt = reinterpret_cast<const int32_t*>(res + P.o_cnt);
  int32_t* slot = reinterpret_cast<int32_t*>(res + P.o_slot);
  int32_t* rec = reinterpret_cast<int32_t*>(res + P.o_rec);
  int best = 0, nrec = 0, overflow = 0;
  for (int k = 0; k < P.n_eval; k++) {
    int s = -1;
    const int c = cnt[k];
    if (c >= P.min_inliers && c > best) {
      best = c;
      if (nrec < PNP_R) {
        s = nrec;
        rec[nrec++] = k;
      } else {
        overflow = 1;
      }
    }
    slot[k] = s;
  }
  int32_t* o = reinterpret_cast<int32_t*>(res + P.o_sel);
  o[5] = nrec;
  o[6] = overflow;
}

// Refine() (:271-316) up to compute_pose: EPnP over the inliers of record slot blockIdx.x.
__global__ __launch_bounds__(64) void k_pnp_refine(const uint8_t* __restrict__ in, uint8_t* __restrict__ res,
                                                   double* __restrict__ ws_all) {
  const PnpDev& P = reinterpret_cast<const PnpDev*>(in)[blockIdx.y];
  const int j = blockIdx.x;  // < PNP_R
  if (j >= reinterpret_cast<const int32_t*>(res + P.o_sel)[5]) return;  // block-uniform
  __shared__ PnpWork work;
  __shared__ double pose[12];
  __shared__ int chosen;
  __shared__ unsigned flg;
  const int lane = threadIdx.x;
  const int k = reinterpret_cast<const int32_t*>(res + P.o_rec)[j];  // written by k_pnp_records: < n_eval
  const int n = P.n;
  const int count = reinterpret_cast<const int32_t*>(res + P.o_cnt)[k];  // <= n: the popcount of the mask below
  double* ws = ws_all + P.ws / 8 + (size_t)j * PNP_WS_DOUBLES * (size_t)n;  // this record's n-point slice
  double* pws = ws;
  double* us = pws + 3 * (size_t)n;
  double* alphas = us + 2 * (size_t)n;
  double* pcs = alphas + 4 * (size_t)n;
  const unsigned long long* mask = reinterpret_cast<const unsigned long long*>(res + P.o_mask) + (size_t)P.words * k;
  const float* p3 = reinterpret_cast<const float*>(in + P.in_p3d);
  const float* p2 = reinterpret_cast<const float*>(in + P.in_p2d);
  int base = 0;  // inliers in the words before this one
  for (int c0 = 0; c0 < n; c0 += 64) {
    const unsigned long long word = mask[c0 >> 6];  // bits at or above n are 0
    const int i = c0 + lane;
    if ((word >> lane) & 1ull) {
      const int pos = base + __popcll(word & ((1ull << lane) - 1ull));  // < count <= n
      pws[3 * pos] = p3[3 * (size_t)i], pws[3 * pos + 1] = p3[3 * (size_t)i + 1], pws[3 * pos + 2] = p3[3 * (size_t)i + 2];
      us[2 * pos] = p2[2 * (size_t)i], us[2 * pos + 1] = p2[2 * (size_t)i + 1];
    }
    base += __popcll(word);
  }
  __threadfence_block();
  __syncthreads();
  pnp_compute_pose(PnpDevGroup<64>(), work, count, pws, us, alphas, pcs, P.K, pose, pose + 9, &chosen, &flg);
  if (lane == 0)
    pnp_store_pose(pose, pose + 9, chosen, flg, reinterpret_cast<double*>(res + P.o_rr) + 9 * (size_t)j,
                   reinterpret_cast<double*>(res + P.o_rt) + 3 * (size_t)j,
                   reinterpret_cast<float*>(res + P.o_rtcw) + 12 * (size_t)j,
                   reinterpret_cast<int32_t*>(res + P.o_rN) + j, reinterpret_cast<uint32_t*>(res + P.o_rflags) + j);
}

// find() (:170-174 over :176-269) per solver from a fresh state, in hypothesis order
__global__ __launch_bounds__(64) void k_pnp_select(const uint8_t* __restrict__ in, uint8_t* __restrict__ res,
                                                   int n_solvers) {
  const int sidx = threadIdx.x;
  if (sidx >= n_solvers) return;
  const PnpDev& P = reinterpret_cast<const PnpDev*>(in)[sidx];
  const int32_t* cnt = reinterpret_cast<const int32_t*>(res + P.o_cnt);
  const int32_t* slot = reinterpret_cast<const int32_t*>(res + P.o_slot);
  const int32_t* rcnt = reinterpret_cast<const int32_t*>(res + P.o_rcnt);
  int iterations = 0, best = -1, best_inliers = 0, accepted = -1, n_inliers = 0;
  while (iterations < P.max_its && iterations < P.n_eval) {
    const int k = iterations++;
    const int c = cnt[k];
    if (c >= P.min_inliers && c > best_inliers) {
      best_inliers = c;
      best = k;
      const int s = slot[k];  // -1 only past PNP_R records, which the host reports
      if (s >= 0 && rcnt[s] > P.min_inliers) {
        accepted = k;
        n_inliers = rcnt[s];
        break;
      }
    }
  }
  int32_t* o = reinterpret_cast<int32_t*>(res + P.o_sel);
  o[0] = accepted;
  o[1] = n_inliers;
  o[2] = best;
  o[3] = best_inliers;
  o[4] = (accepted < 0 && iterations >= P.max_its) ? 1 : 0;
}

// ------------------------------------------------------------------------------------------
// host

struct PnpLast {  // one solver of the last solve, for orbfe_pnp_iterate
  int n = 0, n_eval = 0, min_inliers = 0, max_its = 0, words = 0;
  bool launched = false;
  size_t o_mask = 0, o_tcw = 0, o_cnt = 0, o_slot = 0, o_rmask = 0, o_rtcw = 0, o_rcnt = 0;
};

struct orbfe_pnp : OrbfeDev {
  int S = 0, C = 0, H = 0;
  // inputs (one upload), results (one copy back), the refinement workspace (device only); sized by
  // pnp_plan_bounds
  OrbfeStage in, res, ws;
  std::vector<PnpLast> last;
};

struct PnpParams {
  int min_inliers, max_its;
  float epsilon;
};

// SetRansacParameters (:140-163) in its own float / int / double steps
static PnpParams pnp_ransac_params(int n, double probability, int min_inliers, int max_iterations, int min_set,
                                   float epsilon) {
  PnpParams p;
  int n_min = (int)((float)n * epsilon);  // int nMinInliers = N * mRansacEpsilon
  if (n_min < min_inliers) n_min = min_inliers;
  if (n_min < min_set) n_min = min_set;
  p.min_inliers = n_min;
  if (epsilon < (float)n_min / (float)n) epsilon = (float)n_min / (float)n;
  p.epsilon = epsilon;
  p.max_its = ransac_max_its(n, n_min, epsilon, probability, max_iterations);
  return p;
}

extern "C" int orbfe_pnp_create(int device, int max_solvers, int max_corr, int max_hyp, orbfe_pnp** out) {
  if (!out) return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_pnp_create: bad argument");
  *out = nullptr;
  if (max_solvers < 1 || max_solvers > ORBFE_PNP_MAX_SOLVERS || max_corr < 4 || max_corr > ORBFE_PNP_MAX_CORR ||
      max_hyp < 1 || max_hyp > ORBFE_PNP_MAX_HYP)
    return orbfe_set_error(ORBFE_ERR_ARG,
                           "orbfe_pnp_create: max_solvers in 1..64, max_corr in 4..4096, max_hyp in 1..1024");
  orbfe_pnp* h = new orbfe_pnp();
  h->S = max_solvers;
  h->C = max_corr;
  h->H = max_hyp;
  if (device < 0) {
    *out = h;
    return ORBFE_OK;
  }
  const int st = orbfe_dev_open(h, device, "orbfe_pnp_create");
  if (st != ORBFE_OK) {
    orbfe_pnp_destroy(h);
    return st;
  }
  size_t in_bytes, res_bytes, ws_bytes;
  pnp_plan_bounds(h->S, h->C, h->H, &in_bytes, &res_bytes, &ws_bytes);
  ORBFE_CREATE_HIP(h, orbfe_pnp_destroy, orbfe_stage_alloc(&h->in, in_bytes, true));
  ORBFE_CREATE_HIP(h, orbfe_pnp_destroy, orbfe_stage_alloc(&h->res, res_bytes, true));
  ORBFE_CREATE_HIP(h, orbfe_pnp_destroy, orbfe_stage_alloc(&h->ws, ws_bytes, false));
  *out = h;
  return ORBFE_OK;
}

extern "C" int orbfe_pnp_destroy(orbfe_pnp* h) {
  if (!h) return ORBFE_OK;
  if (orbfe_dev_close(h)) {
    orbfe_stage_free(&h->in);
    orbfe_stage_free(&h->res);
    orbfe_stage_free(&h->ws);
  }
  delete h;
  return ORBFE_OK;
}

// Argument checks of one solver; *n_eval = hypotheses to evaluate (0: n < mRansacMinInliers)
static int pnp_check_solver(const orbfe_pnp* h, const orbfe_pnp_solver_t* s, const orbfe_pnp_result_t* r, int* n_eval,
                            PnpParams* prm) {
  if (s->n < 0 || s->n_hyp < 0 || s->min_inliers < 0 || s->max_iterations < 0 || !(s->probability >= 0.0) ||
      !(s->probability <= 1.0) || !(s->epsilon >= 0.0f && s->epsilon <= 1.0f) || !(s->th2 >= 0.0f && s->th2 < 1e15f))
    return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_pnp_solve_batch: bad solver parameter");
  if (s->min_set != 4)
    return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_pnp_solve_batch: min_set must be 4");
  if (s->n > h->C) return orbfe_set_error(ORBFE_ERR_CAPACITY, "orbfe_pnp_solve_batch: n above the handle's max_corr");
  if (r->hyp_capacity < 0 || r->mask_words < 0 || r->rec_capacity < 0)
    return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_pnp_solve_batch: bad result capacity");
  *n_eval = 0;
  prm->min_inliers = std::max(s->min_inliers, 4);
  prm->max_its = 1;
  prm->epsilon = s->epsilon;
  if (s->n == 0) return ORBFE_OK;  // N < mRansacMinInliers: bNoMore, nothing launched
  *prm = pnp_ransac_params(s->n, s->probability, s->min_inliers, s->max_iterations, s->min_set, s->epsilon);
  if (s->n < prm->min_inliers) return ORBFE_OK;
  if (!s->p3dw || !s->p2d || !s->sigma2)
    return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_pnp_solve_batch: null correspondence array");
  if (s->n_hyp > 0 && !s->rand_idx) return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_pnp_solve_batch: null rand_idx");
  const int e = s->n_hyp;
  if (e > h->H)
    return orbfe_set_error(ORBFE_ERR_CAPACITY, "orbfe_pnp_solve_batch: more hypotheses than the handle's max_hyp");
  const bool per_hyp = r->n_inliers || r->inlier_mask || r->r || r->t || r->tcw || r->n_chosen || r->flags;
  const bool per_rec = r->records || r->refined_inliers || r->refined_mask || r->refined_r || r->refined_t ||
                       r->refined_tcw || r->refined_n_chosen || r->refined_flags;
  if ((per_hyp && e > r->hyp_capacity) || (per_rec && std::min(e, PNP_R) > r->rec_capacity) ||
      (e > 0 && (r->inlier_mask || r->refined_mask) && r->mask_words < (s->n + 63) / 64))
    return orbfe_set_error(ORBFE_ERR_CAPACITY, "orbfe_pnp_solve_batch: result capacity below the evaluated hypotheses");
  for (int i = 0; i < s->n; i++) {
    const float a = s->sigma2[i];
    if (!(a >= 0.0f && a < 1e15f))
      return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_pnp_solve_batch: sigma2 must be finite and >= 0");
  }
  if (!ransac_check_draws(s->rand_idx, e, 4, s->n))
    return orbfe_set_error(ORBFE_ERR_ARG,
                           "orbfe_pnp_solve_batch: rand_idx outside 0 .. n-1-i for draw i of its iteration");
  *n_eval = e;
  return ORBFE_OK;
}

extern "C" int orbfe_pnp_solve_batch(orbfe_pnp* h, const orbfe_pnp_solver_t* solvers, int n_solvers,
                                     orbfe_pnp_result_t* results) {
  if (!h || !solvers || !results || n_solvers < 1)
    return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_pnp_solve_batch: bad argument");
  if (n_solvers > h->S)
    return orbfe_set_error(ORBFE_ERR_CAPACITY, "orbfe_pnp_solve_batch: more solvers than the handle's max_solvers");
  std::vector<int> n_eval(n_solvers);
  std::vector<PnpParams> prm(n_solvers);
  for (int i = 0; i < n_solvers; i++) {
    const int st = pnp_check_solver(h, &solvers[i], &results[i], &n_eval[i], &prm[i]);
    if (st != ORBFE_OK) return st;
  }
  if (h->device < 0) return orbfe_set_error(ORBFE_ERR_STATE, "pnp solver is host-only (device < 0)");
  h->last.assign(n_solvers, PnpLast());
  // plan: the launched solvers' parameter records, then their inputs; results packed the same way
  std::vector<int> act;
  for (int i = 0; i < n_solvers; i++)
    if (n_eval[i] > 0) act.push_back(i);
  const int na = (int)act.size();
  OrbfeStage &in = h->in, &res = h->res, &ws = h->ws;
  in.off = res.off = ws.off = 0;
  PnpDev* dev;
  in.take<PnpDev>((size_t)std::max(na, 1), &dev);
  int max_e = 0;
  for (int a = 0; a < na; a++) {
    const orbfe_pnp_solver_t& s = solvers[act[a]];
    const size_t n = (size_t)s.n, e = (size_t)n_eval[act[a]];
    PnpDev d;
    memset(&d, 0, sizeof(d));
    d.n = s.n;
    d.n_eval = (int)e;
    d.min_inliers = prm[act[a]].min_inliers;
    d.max_its = prm[act[a]].max_its;
    d.words = (s.n + 63) / 64;
    for (int i = 0; i < 4; i++) d.K[i] = (double)s.k[i];  // fu = F.fx ... (:111-114): float widened to double
    pnp_layout(in, res, ws, n, e, d);
    if (in.off > in.cap || res.off > res.cap || ws.off > ws.cap)  // cannot happen within the bounds
      return orbfe_set_error(ORBFE_ERR_CAPACITY, "orbfe_pnp_solve_batch: staging plan exceeds the handle's buffers");
    memcpy(in.h + d.in_p3d, s.p3dw, 12 * n);
    memcpy(in.h + d.in_p2d, s.p2d, 8 * n);
    float* mx = reinterpret_cast<float*>(in.h + d.in_max);
    for (size_t i = 0; i < n; i++) mx[i] = s.sigma2[i] * s.th2;  // mvMaxError (:165-167), float
    memcpy(in.h + d.in_rand, s.rand_idx, 16 * e);
    dev[a] = d;
    max_e = std::max(max_e, (int)e);
    PnpLast& L = h->last[act[a]];
    L.launched = true;
    L.words = d.words;
    L.o_mask = d.o_mask, L.o_tcw = d.o_tcw, L.o_cnt = d.o_cnt, L.o_slot = d.o_slot;
    L.o_rmask = d.o_rmask, L.o_rtcw = d.o_rtcw, L.o_rcnt = d.o_rcnt;
  }
  for (int i = 0; i < n_solvers; i++) {
    PnpLast& L = h->last[i];
    L.n = solvers[i].n;
    L.n_eval = n_eval[i];
    L.min_inliers = prm[i].min_inliers;
    L.max_its = prm[i].max_its;
  }
  if (na > 0) {
    ORBFE_HIP_CHECK(hipSetDevice(h->device));
    int st;
    if ((st = orbfe_stage_upload(&in, h->stream)) != ORBFE_OK) return st;
    const uint8_t* din = in.d;
    uint8_t* dres = res.d;
    double* dws = reinterpret_cast<double*>(ws.d);
    ORBFE_LAUNCH("k_pnp_hypotheses", k_pnp_hypotheses,
                 dim3((max_e + PNP_HYP_PER_BLOCK - 1) / PNP_HYP_PER_BLOCK, na), dim3(64), 0, h->stream, din, dres);
    ORBFE_LAUNCH("k_pnp_inliers", k_pnp_inliers, dim3((max_e + PNP_INL_WAVES - 1) / PNP_INL_WAVES, na),
                 dim3(PNP_INL_THREADS), 0, h->stream, din, dres, 0);
    ORBFE_LAUNCH("k_pnp_records", k_pnp_records, dim3(1), dim3(64), 0, h->stream, din, dres, na);
    ORBFE_LAUNCH("k_pnp_refine", k_pnp_refine, dim3(PNP_R, na), dim3(64), 0, h->stream, din, dres, dws);
    ORBFE_LAUNCH("k_pnp_inliers", k_pnp_inliers, dim3((PNP_R + PNP_INL_WAVES - 1) / PNP_INL_WAVES, na),
                 dim3(PNP_INL_THREADS), 0, h->stream, din, dres, 1);
    ORBFE_LAUNCH("k_pnp_select", k_pnp_select, dim3(1), dim3(64), 0, h->stream, din, dres, na);
    if ((st = orbfe_stage_download(&res, h->stream)) != ORBFE_OK) return st;
  }
  for (int i = 0; i < n_solvers; i++) {
    orbfe_pnp_result_t& r = results[i];
    r.n_records = 0;
    r.n_evaluated = n_eval[i];
    r.ransac_max_its = prm[i].max_its;
    r.ransac_min_inliers = prm[i].min_inliers;
    r.ransac_epsilon = prm[i].epsilon;
    r.accepted = -1;
    r.accepted_inliers = 0;
    r.best = -1;
    r.best_inliers = 0;
    r.no_more = solvers[i].n < prm[i].min_inliers ? 1 : 0;
  }
  for (int a = 0; a < na; a++) {
    const PnpDev& d = dev[a];
    orbfe_pnp_result_t& r = results[act[a]];
    const size_t e = (size_t)d.n_eval;
    const uint8_t* base = res.h;
    const int32_t* sel = reinterpret_cast<const int32_t*>(base + d.o_sel);
    if (sel[6]) {
      h->last.clear();
      return orbfe_set_error(ORBFE_ERR_CAPACITY, "orbfe_pnp_solve_batch: more than ORBFE_PNP_MAX_RECORDS records");
    }
    const size_t nr = (size_t)sel[5];
    if (r.n_inliers) memcpy(r.n_inliers, base + d.o_cnt, 4 * e);
    if (r.r) memcpy(r.r, base + d.o_r, 72 * e);
    if (r.t) memcpy(r.t, base + d.o_t, 24 * e);
    if (r.tcw) memcpy(r.tcw, base + d.o_tcw, 48 * e);
    if (r.n_chosen) memcpy(r.n_chosen, base + d.o_N, 4 * e);
    if (r.flags) memcpy(r.flags, base + d.o_flags, 4 * e);
    if (r.inlier_mask) orbfe_unpack_masks(r.inlier_mask, r.mask_words, base + d.o_mask, d.words, e);
    if (r.records) memcpy(r.records, base + d.o_rec, 4 * nr);
    if (r.refined_inliers) memcpy(r.refined_inliers, base + d.o_rcnt, 4 * nr);
    if (r.refined_r) memcpy(r.refined_r, base + d.o_rr, 72 * nr);
    if (r.refined_t) memcpy(r.refined_t, base + d.o_rt, 24 * nr);
    if (r.refined_tcw) memcpy(r.refined_tcw, base + d.o_rtcw, 48 * nr);
    if (r.refined_n_chosen) memcpy(r.refined_n_chosen, base + d.o_rN, 4 * nr);
    if (r.refined_flags) memcpy(r.refined_flags, base + d.o_rflags, 4 * nr);
    if (r.refined_mask) orbfe_unpack_masks(r.refined_mask, r.mask_words, base + d.o_rmask, d.words, nr);
    r.n_records = (int)nr;
    r.accepted = sel[0];
    r.accepted_inliers = sel[1];
    r.best = sel[2];
    r.best_inliers = sel[3];
    r.no_more = sel[4];
  }
  return ORBFE_OK;
}

extern "C" int orbfe_pnp_iterate(orbfe_pnp* h, int solver_index, int n_iterations, orbfe_pnp_state_t* state,
                                 orbfe_pnp_iterate_t* out) {
  if (!h || !state || !out || n_iterations < 0 || out->mask_words < 0 || state->iterations < 0)
    return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_pnp_iterate: bad argument");
  if (solver_index < 0 || solver_index >= (int)h->last.size())
    return orbfe_set_error(ORBFE_ERR_STATE, "orbfe_pnp_iterate: no such solver in the last solve");
  const PnpLast& L = h->last[solver_index];
  if (out->inlier_mask && out->mask_words < (L.n + 63) / 64)
    return orbfe_set_error(ORBFE_ERR_CAPACITY, "orbfe_pnp_iterate: mask_words below ceil(n / 64)");
  out->returned = 0;
  out->accepted = -1;
  out->no_more = 0;
  out->n_inliers = 0;
  memset(out->tcw, 0, sizeof(out->tcw));
  if (out->inlier_mask) memset(out->inlier_mask, 0, 8 * (size_t)out->mask_words);
  if (L.n < L.min_inliers) {
    out->no_more = 1;
    return ORBFE_OK;
  }
  if (state->best >= L.n_eval) return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_pnp_iterate: state is not this solver's");
  const int32_t* cnt = reinterpret_cast<const int32_t*>(h->res.h + L.o_cnt);
  const int32_t* slot = reinterpret_cast<const int32_t*>(h->res.h + L.o_slot);
  const int32_t* rcnt = reinterpret_cast<const int32_t*>(h->res.h + L.o_rcnt);
  int cur = 0;
  // :193 as written: with ||, a call below mRansacMaxIts runs on to it
  while ((state->iterations < L.max_its || cur < n_iterations) && state->iterations < L.n_eval) {
    cur++;
    const int k = state->iterations++;
    if (cnt[k] >= L.min_inliers) {
      if (cnt[k] > state->best_inliers) {
        state->best_inliers = cnt[k];
        state->best = k;
      }
      // Refine() runs on the best set at every qualifying iteration (:237): from a fresh state it can
      // only succeed at a record's own iteration, after an acceptance it succeeds again
      const int s = state->best >= 0 ? slot[state->best] : -1;
      if (s >= 0 && rcnt[s] > L.min_inliers) {
        out->returned = 1;
        out->accepted = state->best;
        out->n_inliers = rcnt[s];
        memcpy(out->tcw, h->res.h + L.o_rtcw + 48 * (size_t)s, 48);
        if (out->inlier_mask) memcpy(out->inlier_mask, h->res.h + L.o_rmask + 8 * (size_t)L.words * s, 8 * (size_t)L.words);
        return ORBFE_OK;
      }
    }
  }
  if (state->iterations >= L.max_its) {
    out->no_more = 1;
    if (state->best_inliers >= L.min_inliers && state->best >= 0) {
      out->returned = 2;
      out->n_inliers = state->best_inliers;
      memcpy(out->tcw, h->res.h + L.o_tcw + 48 * (size_t)state->best, 48);
      if (out->inlier_mask)
        memcpy(out->inlier_mask, h->res.h + L.o_mask + 8 * (size_t)L.words * state->best, 8 * (size_t)L.words);
    }
  }
  return ORBFE_OK;
}
