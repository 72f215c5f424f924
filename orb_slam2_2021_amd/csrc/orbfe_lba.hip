// orbfe_lba.hip -- Optimizer::LocalBundleAdjustment on the GPU (include/orbfe_lba.h): one local map's
// Levenberg-Marquardt with a Schur complement over the free keyframes.
//
// The Levenberg control flow (lba_run of orbfe_lba_core.h over lm_host_optimize of orbfe_lm_core.h) runs on
// the host and reads one LmRec per linearisation and per trial; the stages are kernels on the handle's
// one stream, each a thread- or lane-per-element call of the core header's functions:
//   k_lba_edge      per active edge: error, robust weight and (linearisation) Jacobians and the edge's
//                   own Hll, bl, Hpl, Hpp, bp products
//   k_lba_point     per point: Hll, bl, chi2 share over its edges in order
//   k_lba_pose      one wavefront per free keyframe: Hpp(i,i), bp_i by the 64-lane rule
//   k_lba_dinv      per point: Dinv = (Hll + lambda I)^-1, db
//   k_lba_schur     one wavefront per (s1 <= s2): the Schur block and, on the diagonal, bschur
//   k_lba_ldlt      one workgroup: the dense LDL^T by columns in global memory and the two solves
//   k_lba_update    per point: back-substitution and the trial point; per keyframe: exp(x) * T
//   k_lba_reduce    one wavefront: the total chi2 with computeLambdaInit's maximum or computeScale
//   k_lba_classify  per edge: chi2 > th || !isDepthPositive
// No kernel waits on another: the stream orders them. Every index a kernel reads was checked by
// orbfe_lba_solve or built by lba_plan / lba_active; every loop runs to a count among those.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>
#include <vector>

#include "../../include/orbfe_lba.h"
#include "orbfe_device.h"
#include "orbfe_ktimer.h"
#include "orbfe_lba_core.h"

static_assert(LM_FLAG_LARGE_STEP == ORBFE_LBA_FLAG_LARGE_STEP && LM_FLAG_NONFINITE == ORBFE_LBA_FLAG_NONFINITE, "flag values");
static_assert(LM_STOP_ALL == ORBFE_LBA_STOP_ALL && LM_STOP_TERMINATE == ORBFE_LBA_STOP_TERMINATE &&
                  LM_STOP_NBAD == ORBFE_LBA_STOP_NBAD && LM_STOP_NO_EDGE == ORBFE_LBA_STOP_NO_EDGE &&
                  LM_STOP_FLAG == ORBFE_LBA_STOP_FLAG,
              "stop codes");
static_assert(sizeof(LbaRound) == sizeof(orbfe_lba_round_t), "trace layout");
static_assert(LBA_MAX_FREE == ORBFE_LBA_MAX_FREE_KF, "free keyframe cap");

#define LBA_BLOCK 128
#define LBA_LDLT_THREADS 256
#define LBA_LDLT_ROWS 3  // rows of one column a thread owns
static_assert(6 * LBA_MAX_FREE <= LBA_LDLT_ROWS * LBA_LDLT_THREADS, "k_lba_ldlt covers a column in one pass");

template <bool FULL>
__global__ __launch_bounds__(LBA_BLOCK) void k_lba_edge(LbaWs w, int trial) {
  const int e = blockIdx.x * LBA_BLOCK + threadIdx.x;
  if (e < w.ne) lba_edge<FULL>(w, e, trial != 0);
}

template <bool FULL>
__global__ __launch_bounds__(LBA_BLOCK) void k_lba_point(LbaWs w) {
  const int p = blockIdx.x * LBA_BLOCK + threadIdx.x;
  if (p < w.np) lba_point_sum<FULL>(w, p);
}

// the tree: lane 0 ends with s[0] of the host's s[l] += s[l + stride]
__device__ inline double lba_tree(double v) {
#pragma unroll
  for (int stride = LBA_LANES / 2; stride >= 1; stride >>= 1) v = v + __shfl_down(v, stride);
  return v;
}

__global__ __launch_bounds__(LBA_LANES) void k_lba_pose(LbaWs w) {
  const int f = w.free_of_slot[blockIdx.x];
  double acc[27];
  lba_pose_lane(w, f, threadIdx.x, acc);
#pragma unroll
  for (int k = 0; k < 27; k++) acc[k] = lba_tree(acc[k]);
  if (threadIdx.x == 0) lba_pose_finish(w, f, acc);
}

__global__ __launch_bounds__(LBA_BLOCK) void k_lba_dinv(LbaWs w, double lambda) {
  const int p = blockIdx.x * LBA_BLOCK + threadIdx.x;
  if (p < w.np) lba_point_dinv(w, p, lambda);
}

__global__ __launch_bounds__(LBA_LANES) void k_lba_schur(LbaWs w, double lambda) {
  const int s1 = blockIdx.y, s2 = blockIdx.x;
  if (s1 > s2) return;
  double acc[42];
  lba_schur_lane(w, w.free_of_slot[s1], w.free_of_slot[s2], threadIdx.x, acc);
#pragma unroll
  for (int k = 0; k < 42; k++) acc[k] = lba_tree(acc[k]);
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

__global__ __launch_bounds__(LBA_BLOCK) void k_lba_update(LbaWs w) {
  const int i = blockIdx.x * LBA_BLOCK + threadIdx.x;
  if (i < w.np) {
    if (!w.rec->fail) lba_point_backsub(w, i);  // after a failed solve x keeps its last values
    lba_update_point(w, i);
  } else if (i - w.np < w.nk) {
    lba_update_kf(w, i - w.np);
  }
}

__global__ __launch_bounds__(LBA_LANES) void k_lba_reduce(LbaWs w, int mode, double lambda) {
  double part[2];
  lba_reduce_lane(w, threadIdx.x, mode, lambda, part);
  const double chi = lba_tree(part[0]);
  double other;
  if (mode) {
    other = lba_tree(part[1]);
  } else {
    other = part[1];
#pragma unroll
    for (int stride = LBA_LANES / 2; stride >= 1; stride >>= 1) {
      const double o = __shfl_down(other, stride);
      other = o > other ? o : other;
    }
  }
  if (threadIdx.x == 0) lba_reduce_finish(w, mode, lambda, chi, other);
}

__global__ __launch_bounds__(LBA_BLOCK) void k_lba_classify(LbaWs w, uint8_t* flag) {
  const int e = blockIdx.x * LBA_BLOCK + threadIdx.x;
  if (e < w.ne) flag[e] = lba_edge_flag(w, e) ? 1 : 0;
}

// ------------------------------------------------------------------------------------------
// host

struct orbfe_lba {
  int device = -1;
  int max_free = 0, max_kf = 0, max_points = 0, max_edges = 0;
  hipStream_t stream = nullptr;
  uint8_t* d_pool = nullptr;
  size_t pool_bytes = 0;
  LmRec* h_rec = nullptr;  // pinned
  LbaWs w;                  // device pointers, sized for the handle's bounds
  uint8_t* d_flag = nullptr;
};

static size_t lba_al(size_t b) { return (b + 255) & ~(size_t)255; }

// carves the device pool; with base == nullptr only the size is computed
static size_t lba_carve(orbfe_lba* h, uint8_t* base) {
  size_t off = 0;
  const size_t nk = h->max_kf, nf = h->max_free, np = h->max_points, ne = h->max_edges, n = 6 * nf;
  LbaWs& w = h->w;
  auto take = [&](size_t bytes) {
    uint8_t* p = base ? base + off : nullptr;
    off += lba_al(bytes);
    return p;
  };
#define LBA_TAKE(field, type, count) w.field = reinterpret_cast<type*>(take(sizeof(type) * (count)))
  LBA_TAKE(cam, const double, 5 * nk);
  LBA_TAKE(kf_free, const int, nk);
  LBA_TAKE(edge_begin, const int, np + 1);
  LBA_TAKE(e_kf, const int, ne);
  LBA_TAKE(e_pt, const int, ne);
  LBA_TAKE(e_obs, const double, 3 * ne);
  LBA_TAKE(e_w, const double, ne);
  LBA_TAKE(e_stereo, const uint8_t, ne);
  LBA_TAKE(kl_begin, const int, nf * LBA_LANES + 1);
  LBA_TAKE(kl_edge, const int, ne);
  LBA_TAKE(e_active, const uint8_t, ne);
  LBA_TAKE(p_active, const uint8_t, np);
  LBA_TAKE(slot_of_free, const int, nf);
  LBA_TAKE(free_of_slot, const int, nf);
  LBA_TAKE(est_T, double, 7 * nk);
  LBA_TAKE(tri_T, double, 7 * nk);
  LBA_TAKE(est_X, double, 3 * np);
  LBA_TAKE(tri_X, double, 3 * np);
  LBA_TAKE(e_err, double, 3 * ne);
  LBA_TAKE(e_prod, double, LBA_EDGE_DOUBLES * ne);
  LBA_TAKE(p_hll, double, 9 * np);
  LBA_TAKE(p_bl, double, 3 * np);
  LBA_TAKE(p_chi, double, np);
  LBA_TAKE(p_dinv, double, 9 * np);
  LBA_TAKE(p_db, double, 3 * np);
  LBA_TAKE(p_xl, double, 3 * np);
  LBA_TAKE(hpp, double, 21 * nf);
  LBA_TAKE(bp, double, 6 * nf);
  LBA_TAKE(S, double, n * n);
  LBA_TAKE(bs, double, n);
  LBA_TAKE(Lm, double, n * n);
  LBA_TAKE(Mm, double, n * n);
  LBA_TAKE(d, double, n);
  LBA_TAKE(y, double, n);
  LBA_TAKE(xp, double, n);
  LBA_TAKE(rec, LmRec, 1);
#undef LBA_TAKE
  h->d_flag = take(ne);
  return off;
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
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device >= ndev) {
    delete h;
    return orbfe_set_error(ORBFE_ERR_HIP, "orbfe_lba_create: no such HIP device");
  }
  h->device = device;
  h->pool_bytes = lba_carve(h, nullptr);
  auto fail = [&](hipError_t e, const char* what) {
    const int st = orbfe_set_hip_error(e, what);
    orbfe_lba_destroy(h);
    return st;
  };
#define LBA_TRY(expr)                             \
  do {                                            \
    hipError_t _e = (expr);                       \
    if (_e != hipSuccess) return fail(_e, #expr); \
  } while (0)
  LBA_TRY(hipSetDevice(device));
  LBA_TRY(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  LBA_TRY(hipMalloc(&h->d_pool, h->pool_bytes));
  LBA_TRY(hipHostMalloc(&h->h_rec, sizeof(LmRec), hipHostMallocDefault));
#undef LBA_TRY
  lba_carve(h, h->d_pool);
  *out = h;
  return ORBFE_OK;
}

extern "C" int orbfe_lba_destroy(orbfe_lba* h) {
  if (!h) return ORBFE_OK;
  if (h->device >= 0) {
    hipSetDevice(h->device);
    if (h->stream) hipStreamSynchronize(h->stream);
    hipFree(h->d_pool);
    if (h->h_rec) hipHostFree(h->h_rec);
    if (h->stream) hipStreamDestroy(h->stream);
  }
  delete h;
  return ORBFE_OK;
}

namespace {
inline unsigned lba_grid(int n) { return (unsigned)((n + LBA_BLOCK - 1) / LBA_BLOCK); }

// lba_run's backend over the handle's device workspace
struct LbaDevBackend {
  orbfe_lba* h;
  LbaWs w;

  template <class T>
  int up(const T* dst, const T* src, size_t count) {
    if (count == 0) return ORBFE_OK;
    ORBFE_HIP_CHECK(hipMemcpyAsync(const_cast<T*>(dst), src, sizeof(T) * count, hipMemcpyHostToDevice, h->stream));
    ORBFE_HIP_CHECK(hipStreamSynchronize(h->stream));  // the source may be pageable and short-lived
    return ORBFE_OK;
  }

  int start(const LbaPlan& P) {
    w = h->w;
    w.nk = P.nk, w.nfree = P.nfree, w.np = P.np, w.ne = P.ne, w.nslot = 0, w.kernel_on = 1;
    lba_set_deltas(&w);
    int st;
#define LBA_UP(dst, src, count) \
  if ((st = up(dst, src, count)) != ORBFE_OK) return st
    LBA_UP(w.cam, P.cam.data(), P.cam.size());
    LBA_UP(w.kf_free, P.kf_free.data(), P.kf_free.size());
    LBA_UP(w.edge_begin, P.edge_begin, (size_t)P.np + 1);
    LBA_UP(w.e_kf, P.e_kf, (size_t)P.ne);
    LBA_UP(w.e_pt, P.e_pt.data(), P.e_pt.size());
    LBA_UP(w.e_obs, P.e_obs.data(), P.e_obs.size());
    LBA_UP(w.e_w, P.e_w.data(), P.e_w.size());
    LBA_UP(w.e_stereo, P.e_stereo.data(), P.e_stereo.size());
    LBA_UP(w.kl_begin, P.kl_begin.data(), P.kl_begin.size());
    LBA_UP(w.kl_edge, P.kl_edge.data(), P.kl_edge.size());
    LBA_UP((const double*)w.est_T, P.T0.data(), P.T0.size());
    LBA_UP((const double*)w.tri_T, P.T0.data(), P.T0.size());
    LBA_UP((const double*)w.est_X, P.X0.data(), P.X0.size());
    LBA_UP((const double*)w.tri_X, P.X0.data(), P.X0.size());
    ORBFE_HIP_CHECK(hipMemsetAsync(w.e_err, 0, sizeof(double) * 3 * (size_t)P.ne, h->stream));
    return ORBFE_OK;
  }

  int begin_round(const LbaActive& A, bool kernel_on) {
    int st;
    LBA_UP(w.e_active, A.e_active.data(), A.e_active.size());
    LBA_UP(w.p_active, A.p_active.data(), A.p_active.size());
    LBA_UP(w.slot_of_free, A.slot_of_free.data(), A.slot_of_free.size());
    LBA_UP(w.free_of_slot, A.free_of_slot.data(), A.free_of_slot.size());
#undef LBA_UP
    w.nslot = A.nslot, w.kernel_on = kernel_on ? 1 : 0;
    ORBFE_HIP_CHECK(hipMemsetAsync(w.xp, 0, sizeof(double) * 6 * (size_t)w.nfree, h->stream));
    ORBFE_HIP_CHECK(hipMemsetAsync(w.p_xl, 0, sizeof(double) * 3 * (size_t)w.np, h->stream));
    return ORBFE_OK;
  }

  int read_rec(LmRec* out) {
    ORBFE_HIP_CHECK(hipGetLastError());
    ORBFE_HIP_CHECK(hipMemcpyAsync(h->h_rec, w.rec, sizeof(LmRec), hipMemcpyDeviceToHost, h->stream));
    ORBFE_HIP_CHECK(hipStreamSynchronize(h->stream));
    *out = *h->h_rec;
    return ORBFE_OK;
  }

  int linearize(LmRec* out) {
    ORBFE_HIP_CHECK(hipMemsetAsync(w.rec, 0, sizeof(LmRec), h->stream));
    ORBFE_LAUNCH("k_lba_edge", k_lba_edge<true>, dim3(lba_grid(w.ne)), dim3(LBA_BLOCK), 0, h->stream, w, 0);
    ORBFE_LAUNCH("k_lba_point", k_lba_point<true>, dim3(lba_grid(w.np)), dim3(LBA_BLOCK), 0, h->stream, w);
    if (w.nslot > 0) ORBFE_LAUNCH("k_lba_pose", k_lba_pose, dim3(w.nslot), dim3(LBA_LANES), 0, h->stream, w);
    ORBFE_LAUNCH("k_lba_reduce", k_lba_reduce, dim3(1), dim3(LBA_LANES), 0, h->stream, w, 0, 0.0);
    return read_rec(out);
  }

  int trial(double lambda, LmRec* out) {
    ORBFE_HIP_CHECK(hipMemsetAsync(w.rec, 0, sizeof(LmRec), h->stream));
    ORBFE_LAUNCH("k_lba_dinv", k_lba_dinv, dim3(lba_grid(w.np)), dim3(LBA_BLOCK), 0, h->stream, w, lambda);
    if (w.nslot > 0)
      ORBFE_LAUNCH("k_lba_schur", k_lba_schur, dim3(w.nslot, w.nslot), dim3(LBA_LANES), 0, h->stream, w, lambda);
    ORBFE_LAUNCH("k_lba_ldlt", k_lba_ldlt, dim3(1), dim3(LBA_LDLT_THREADS), 0, h->stream, w);
    ORBFE_LAUNCH("k_lba_update", k_lba_update, dim3(lba_grid(w.np + w.nk)), dim3(LBA_BLOCK), 0, h->stream, w);
    ORBFE_LAUNCH("k_lba_edge_trial", k_lba_edge<false>, dim3(lba_grid(w.ne)), dim3(LBA_BLOCK), 0, h->stream, w, 1);
    ORBFE_LAUNCH("k_lba_point_chi", k_lba_point<false>, dim3(lba_grid(w.np)), dim3(LBA_BLOCK), 0, h->stream, w);
    ORBFE_LAUNCH("k_lba_reduce", k_lba_reduce, dim3(1), dim3(LBA_LANES), 0, h->stream, w, 1, lambda);
    return read_rec(out);
  }

  int accept() {  // discardTop: the trial estimates become the accepted ones
    double* t = w.est_T;
    w.est_T = w.tri_T, w.tri_T = t;
    t = w.est_X;
    w.est_X = w.tri_X, w.tri_X = t;
    return ORBFE_OK;
  }

  int classify(uint8_t* flag) {
    ORBFE_LAUNCH("k_lba_classify", k_lba_classify, dim3(lba_grid(w.ne)), dim3(LBA_BLOCK), 0, h->stream, w, h->d_flag);
    ORBFE_HIP_CHECK(hipGetLastError());
    ORBFE_HIP_CHECK(hipMemcpyAsync(flag, h->d_flag, (size_t)w.ne, hipMemcpyDeviceToHost, h->stream));
    ORBFE_HIP_CHECK(hipStreamSynchronize(h->stream));
    return ORBFE_OK;
  }

  int finish(double* T, double* X) {
    ORBFE_HIP_CHECK(hipMemcpyAsync(T, w.est_T, sizeof(double) * 7 * (size_t)w.nk, hipMemcpyDeviceToHost, h->stream));
    ORBFE_HIP_CHECK(hipMemcpyAsync(X, w.est_X, sizeof(double) * 3 * (size_t)w.np, hipMemcpyDeviceToHost, h->stream));
    ORBFE_HIP_CHECK(hipStreamSynchronize(h->stream));
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
  if (p->edge_begin[0] != 0 || p->edge_begin[p->n_points] != p->n_edges)
    return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_lba_solve: edge_begin is not a CSR over n_edges");
  std::vector<int> seen(p->n_kf > 0 ? p->n_kf : 1, -1);
  for (int q = 0; q < p->n_points; q++) {
    const int b = p->edge_begin[q], e = p->edge_begin[q + 1];
    if (b > e || b < 0 || e > p->n_edges) return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_lba_solve: edge_begin is not a CSR over n_edges");
    for (int i = b; i < e; i++) {
      const int kf = p->edge_kf[i];
      if (kf < 0 || kf >= p->n_kf) return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_lba_solve: keyframe index out of range");
      if (seen[kf] == q) return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_lba_solve: a keyframe listed twice under one point");
      seen[kf] = q;
    }
  }
  return ORBFE_OK;
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
  LbaDevBackend b = {h, h->w};
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
