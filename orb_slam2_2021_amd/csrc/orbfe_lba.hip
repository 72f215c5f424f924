// orbfe_lba.hip -- Optimizer::LocalBundleAdjustment on the GPU (include/orbfe_lba.h): one local map's
// Levenberg-Marquardt with a Schur complement over the free keyframes.
//
// The Levenberg control flow (lba_run of orbfe_lba_core.h over lm_host_optimize of orbfe_lm_core.h) runs on
// the host and reads one LmRec per linearisation and per trial; the stages are kernels on the handle's
// one stream, each a thread- or lane-per-element call of the core header's functions. Those marked *
// are orbfe_ba_device.h's k_ba_* kernels, the one set this file and orbfe_gba.hip both launch, under this
// file's labels for the kernel timer:
//   k_lba_edge*     per active edge: error, robust weight and (linearisation) Jacobians and the edge's
//                   own Hll, bl, Hpl, Hpp, bp products
//   k_lba_point*    per point: Hll, bl, chi2 share over its edges in order
//   k_lba_pose*     one wavefront per free keyframe: Hpp(i,i), bp_i by the 64-lane rule
//   k_lba_dinv*     per point: Dinv = (Hll + lambda I)^-1, db
//   k_lba_schur     one wavefront per (s1 <= s2): the Schur block and, on the diagonal, bschur
//   k_lba_ldlt      one workgroup: the dense LDL^T by columns in global memory and the two solves
//   k_lba_update*   per point: back-substitution and the trial point; per keyframe: exp(x) * T
//   k_lba_reduce*   one wavefront: the total chi2 with computeLambdaInit's maximum or computeScale
//   k_lba_classify  per edge: chi2 > th || !isDepthPositive
// No kernel waits on another: the stream orders them. Every index a kernel reads was checked by
// orbfe_lba_solve or built by lba_plan / lba_active; every loop runs to a count among those.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>
#include <vector>

#include "../../include/orbfe_lba.h"
#include "orbfe_ba_device.h"

static_assert(LM_FLAG_LARGE_STEP == ORBFE_LBA_FLAG_LARGE_STEP && LM_FLAG_NONFINITE == ORBFE_LBA_FLAG_NONFINITE, "flag values");
static_assert(LM_STOP_ALL == ORBFE_LBA_STOP_ALL && LM_STOP_TERMINATE == ORBFE_LBA_STOP_TERMINATE &&
                  LM_STOP_NBAD == ORBFE_LBA_STOP_NBAD && LM_STOP_NO_EDGE == ORBFE_LBA_STOP_NO_EDGE &&
                  LM_STOP_FLAG == ORBFE_LBA_STOP_FLAG,
              "stop codes");
static_assert(sizeof(LbaRound) == sizeof(orbfe_lba_round_t), "trace layout");
static_assert(LBA_MAX_FREE == ORBFE_LBA_MAX_FREE_KF, "free keyframe cap");

#define LBA_LDLT_THREADS 256
#define LBA_LDLT_ROWS 3  // rows of one column a thread owns
static_assert(6 * LBA_MAX_FREE <= LBA_LDLT_ROWS * LBA_LDLT_THREADS, "k_lba_ldlt covers a column in one pass");

__global__ __launch_bounds__(LBA_LANES) void k_lba_schur(LbaWs w, double lambda) {
  const int s1 = blockIdx.y, s2 = blockIdx.x;
  if (s1 > s2) return;
  double acc[42];
  lba_schur_lane(w, w.free_of_slot[s1], w.free_of_slot[s2], threadIdx.x, acc);
#pragma unroll
  for (int k = 0; k < 42; k++) acc[k] = ba_tree(acc[k]);
  if (threadIdx.x == 0) lba_schur_finish(w, s1, s2, lambda, acc);
}

// Column j: every row i >= j takes its dot product (lba_ldlt_dot) against the finished columns, row j's is
// d_j; then the rows below divide. The same per-element order as the host's loop. The solves update all
// rows per k, which keeps each row's k ascending (forward) and descending (backward).
__global__ __launch_bounds__(LBA_LDLT_THREADS) void k_lba_ldlt(LbaWs w) {
  const int n = 6 * w.nslot, tid = threadIdx.x;
  __shared__ double s_d;
  __shared__ int s_fail;
  __shared__ double sy[6 * LBA_MAX_FREE];
  if (tid == 0) s_fail = w.rec->fail;
  __syncthreads();
  if (s_fail) return;
  for (int j = 0; j < n; j++) {
    double v[LBA_LDLT_ROWS];
#pragma unroll
    for (int c = 0; c < LBA_LDLT_ROWS; c++) {
      const int i = j + tid + c * LBA_LDLT_THREADS;
      v[c] = i < n ? lba_ldlt_dot(w, n, i, j) : 0.0;
    }
    if (tid == 0) s_d = v[0];
    __syncthreads();
    const double dj = s_d;
    if (!po_finite(dj) || dj == 0.0) {  // the same dj in every thread
      if (tid == 0) lm_fail(w.rec, po_finite(dj) ? 0u : LM_FLAG_NONFINITE);
      return;
    }
#pragma unroll
    for (int c = 0; c < LBA_LDLT_ROWS; c++) {
      const int i = j + tid + c * LBA_LDLT_THREADS;
      if (i == j) {
        w.d[j] = dj;
      } else if (i < n) {
        const double l = v[c] / dj;
        w.Lm[(size_t)j * n + i] = l;
        w.Mm[(size_t)j * n + i] = l * dj;
      }
    }
    __syncthreads();
  }
  for (int i = tid; i < n; i += LBA_LDLT_THREADS) sy[i] = w.bs[i];
  __syncthreads();
  for (int k = 0; k < n; k++) {
    const double yk = sy[k];
    for (int i = k + 1 + tid; i < n; i += LBA_LDLT_THREADS) sy[i] = sy[i] - w.Lm[(size_t)k * n + i] * yk;
    __syncthreads();
  }
  for (int i = tid; i < n; i += LBA_LDLT_THREADS) sy[i] = sy[i] / w.d[i];
  __syncthreads();
  for (int k = n - 1; k >= 0; k--) {
    const double xk = sy[k];
    for (int i = tid; i < k; i += LBA_LDLT_THREADS) sy[i] = sy[i] - w.Lm[(size_t)i * n + k] * xk;
    __syncthreads();
  }
  for (int i = tid; i < n; i += LBA_LDLT_THREADS) w.xp[i] = sy[i];
}

__global__ __launch_bounds__(BA_BLOCK) void k_lba_classify(LbaWs w, uint8_t* flag) {
  const int e = blockIdx.x * BA_BLOCK + threadIdx.x;
  if (e < w.ne) flag[e] = lba_edge_flag(w, e) ? 1 : 0;
}

// ------------------------------------------------------------------------------------------
// host

struct orbfe_lba : OrbfeDev {
  int max_free = 0, max_kf = 0, max_points = 0, max_edges = 0;
  uint8_t* d_pool = nullptr;
  size_t pool_bytes = 0;
  LmRec* h_rec = nullptr;  // pinned
  LbaWs w;                  // device pointers, sized for the handle's bounds
  uint8_t* d_flag = nullptr;
};

// carves the device pool; with base == nullptr only the size is computed
static size_t lba_carve(orbfe_lba* h, uint8_t* base) {
  OrbfeStage pool;
  pool.d = base;
  ba_carve(pool, h->w, h->max_kf, h->max_free, h->max_points, h->max_edges, true);
  pool.take(h->d_flag, h->max_edges);
  return pool.off;
}

extern "C" int orbfe_lba_create(int device, int max_free_kf, int max_kf, int max_points, int max_edges, orbfe_lba** out) {
  if (!out) return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_lba_create: bad argument");
  *out = nullptr;
  if (max_free_kf < 1 || max_free_kf > ORBFE_LBA_MAX_FREE_KF || max_kf < max_free_kf || max_kf > ORBFE_LBA_MAX_KF ||
      max_points < 1 || max_points > ORBFE_LBA_MAX_POINTS || max_edges < 1 || max_edges > ORBFE_LBA_MAX_EDGES)
    return orbfe_set_error(ORBFE_ERR_ARG,
                           "orbfe_lba_create: max_free_kf in 1..128, max_kf in max_free_kf..512, max_points in 1..16384, "
                           "max_edges in 1..131072");
  orbfe_lba* h = new orbfe_lba();
  memset(&h->w, 0, sizeof(h->w));
  h->max_free = max_free_kf, h->max_kf = max_kf, h->max_points = max_points, h->max_edges = max_edges;
  if (device < 0) {
    *out = h;
    return ORBFE_OK;
  }
  const int open_st = orbfe_dev_open(h, device, "orbfe_lba_create");
  if (open_st != ORBFE_OK) {
    orbfe_lba_destroy(h);
    return open_st;
  }
  h->pool_bytes = lba_carve(h, nullptr);
  ORBFE_CREATE_HIP(h, orbfe_lba_destroy, hipMalloc(&h->d_pool, h->pool_bytes));
  ORBFE_CREATE_HIP(h, orbfe_lba_destroy, hipHostMalloc(&h->h_rec, sizeof(LmRec), hipHostMallocDefault));
  lba_carve(h, h->d_pool);
  *out = h;
  return ORBFE_OK;
}

extern "C" int orbfe_lba_destroy(orbfe_lba* h) {
  if (!h) return ORBFE_OK;
  if (orbfe_dev_close(h)) {
    hipFree(h->d_pool);
    if (h->h_rec) hipHostFree(h->h_rec);
  }
  delete h;
  return ORBFE_OK;
}

namespace {
const BaNames kLbaNames = {"k_lba_edge",   "k_lba_point",      "k_lba_pose",      "k_lba_dinv",
                           "k_lba_update", "k_lba_edge_trial", "k_lba_point_chi", "k_lba_reduce"};

// lba_run's backend: BaDevBackend with the dense Schur complement, k_lba_ldlt and the classification
struct LbaDevBackend : BaDevBackend {
  orbfe_lba* h;

  int start(const LbaPlan& P) {
    w = h->w;
    lba_set_deltas(&w);
    return BaDevBackend::start(P);
  }

  int begin_round(const LbaActive& A, bool kernel_on) { return BaDevBackend::begin_round(A, kernel_on, 6 * (size_t)w.nfree); }

  int trial(double lambda, LmRec* out) {
    int st = begin_trial(lambda);
    if (st != ORBFE_OK) return st;
    if (w.nslot > 0)
      ORBFE_LAUNCH("k_lba_schur", k_lba_schur, dim3(w.nslot, w.nslot), dim3(LBA_LANES), 0, stream, w, lambda);
    ORBFE_LAUNCH("k_lba_ldlt", k_lba_ldlt, dim3(1), dim3(LBA_LDLT_THREADS), 0, stream, w);
    return end_trial(lambda, out);
  }

  int classify(uint8_t* flag) {
    ORBFE_LAUNCH("k_lba_classify", k_lba_classify, dim3(ba_grid(w.ne)), dim3(BA_BLOCK), 0, stream, w, h->d_flag);
    ORBFE_HIP_CHECK(hipGetLastError());
    ORBFE_HIP_CHECK(hipMemcpyAsync(flag, h->d_flag, (size_t)w.ne, hipMemcpyDeviceToHost, stream));
    ORBFE_HIP_CHECK(hipStreamSynchronize(stream));
    return ORBFE_OK;
  }
};
}  // namespace

// the boundary: everything a kernel will use as an index
static int lba_check(const orbfe_lba* h, const orbfe_lba_problem_t* p, const orbfe_lba_result_t* r) {
  if (p->n_kf < 0 || p->n_points < 0 || p->n_edges < 0 || r->mask_words < 0)
    return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_lba_solve: negative count");
  if (p->n_kf > h->max_kf || p->n_points > h->max_points || p->n_edges > h->max_edges)
    return orbfe_set_error(ORBFE_ERR_CAPACITY, "orbfe_lba_solve: problem above the handle's bounds");
  if ((r->erase_mask || r->level1_mask) && r->mask_words < (p->n_edges + 63) / 64)
    return orbfe_set_error(ORBFE_ERR_CAPACITY, "orbfe_lba_solve: mask_words below ceil(n_edges / 64)");
  if (!p->edge_begin || (p->n_kf > 0 && (!p->tcw || !p->k || !p->bf || !p->fixed || !r->tcw)) ||
      (p->n_points > 0 && (!p->xw || !r->xw)) || (p->n_edges > 0 && (!p->edge_kf || !p->kp_un || !p->u_right || !p->inv_sigma2)))
    return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_lba_solve: null array");
  if (p->stop_at_poll < -1) return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_lba_solve: stop_at_poll below -1");
  int nfree = 0;
  for (int i = 0; i < p->n_kf; i++) nfree += p->fixed[i] ? 0 : 1;
  if (nfree > h->max_free) return orbfe_set_error(ORBFE_ERR_CAPACITY, "orbfe_lba_solve: free keyframes above the handle's bound");
  return ba_check_csr("orbfe_lba_solve", p->n_kf, p->n_points, p->n_edges, p->edge_begin, p->edge_kf);
}

extern "C" int orbfe_lba_solve(orbfe_lba* h, const orbfe_lba_problem_t* p, orbfe_lba_result_t* r) {
  if (!h || !p || !r) return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_lba_solve: bad argument");
  int st = lba_check(h, p, r);
  if (st != ORBFE_OK) return st;
  if (h->device < 0) return orbfe_set_error(ORBFE_ERR_STATE, "local bundle adjuster is host-only (device < 0)");
  LbaIn in = {p->n_kf, p->n_points, p->n_edges, p->tcw, p->k, p->bf, p->fixed, p->xw, p->edge_begin, p->edge_kf,
              p->kp_un, p->u_right, p->inv_sigma2, p->stop_flag, p->stop_at_poll};
  LbaPlan plan;
  lba_plan(in, &plan);
  LbaOut o;
  ORBFE_HIP_CHECK(hipSetDevice(h->device));
  LbaDevBackend b = {{h->stream, h->h_rec, h->w, &kLbaNames}, h};
  st = lba_run(b, in, plan, &o);
  if (st != ORBFE_OK) return st;
  if (p->n_kf > 0) memcpy(r->tcw, o.tcw.data(), sizeof(float) * o.tcw.size());
  if (p->n_points > 0) memcpy(r->xw, o.xw.data(), sizeof(float) * o.xw.size());
  for (int m = 0; m < 2; m++) {
    uint64_t* mask = m ? r->level1_mask : r->erase_mask;
    const std::vector<uint8_t>& bits = m ? o.level1 : o.erase;
    if (!mask) continue;
    for (int i = 0; i < r->mask_words; i++) mask[i] = 0;
    for (int e = 0; e < p->n_edges; e++)
      if (bits[e]) mask[e >> 6] |= 1ull << (e & 63);
  }
  r->n_erase = o.n_erase, r->rounds_run = o.rounds_run, r->flags = o.flags, r->polls = o.polls;
  memcpy(r->rounds, o.rounds, sizeof(r->rounds));
  return ORBFE_OK;
}
