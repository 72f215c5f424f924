// orbfe_gba.hip -- Optimizer::BundleAdjustment on the GPU (include/orbfe_gba.h): a whole map's
// Levenberg-Marquardt, the Schur complement over the covisible keyframe pairs, the reduced system a 6x6
// block envelope factorised across workgroups.
//
// The Levenberg control flow (gba_run of orbfe_gba_core.h over lm_host_optimize) runs on the host and
// reads one LmRec per linearisation and per trial; the stages are kernels on the handle's one stream:
//   k_gba_edge / point / pose / dinv / update / reduce   the stages of orbfe_lba.hip over the same core
//   k_gba_schur     one wavefront per structural pair: the Schur block into the envelope's lower triangle
//                   and, on the diagonal pairs, bschur
//   k_gba_pivot     per pivot block, one workgroup: the 6x6 diagonal factorisation, then the column below
//                   it scaled, one scalar row per thread
//   k_gba_trailing  per pivot block, grid-wide: one thread per scalar of one (a, bb) block of the column's
//                   rows, its six updates in ascending p
//   k_gba_subst     one workgroup: the forward and the backward substitution over the envelope
// k_gba_pivot and k_gba_trailing are orbfe_essgraph.hip's k_eg_factor split at its two __syncthreads()
// boundaries. No kernel waits on another workgroup: the stream orders them, about 2 n_slots launches per
// trial. Every index a kernel reads was checked by orbfe_gba_solve or built by lba_plan / lba_active /
// gba_plan_envelope; every loop runs to a count among those.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>
#include <vector>

#include "../../include/orbfe_gba.h"
#include "orbfe_device.h"
#include "orbfe_gba_core.h"
#include "orbfe_ktimer.h"

static_assert(LM_FLAG_LARGE_STEP == ORBFE_GBA_FLAG_LARGE_STEP && LM_FLAG_NONFINITE == ORBFE_GBA_FLAG_NONFINITE, "flag values");
static_assert(LM_STOP_ALL == ORBFE_GBA_STOP_ALL && LM_STOP_TERMINATE == ORBFE_GBA_STOP_TERMINATE &&
                  LM_STOP_NBAD == ORBFE_GBA_STOP_NBAD && LM_STOP_NO_EDGE == ORBFE_GBA_STOP_NO_EDGE &&
                  LM_STOP_FLAG == ORBFE_GBA_STOP_FLAG,
              "stop codes");
static_assert(sizeof(GbaTrace) == sizeof(orbfe_gba_trace_t), "trace layout");

#define GBA_BLOCK 128
#define GBA_FACTOR_THREADS 256

template <bool FULL>
__global__ __launch_bounds__(GBA_BLOCK) void k_gba_edge(LbaWs w, int trial) {
  const int e = blockIdx.x * GBA_BLOCK + threadIdx.x;
  if (e < w.ne) lba_edge<FULL>(w, e, trial != 0);
}

template <bool FULL>
__global__ __launch_bounds__(GBA_BLOCK) void k_gba_point(LbaWs w) {
  const int p = blockIdx.x * GBA_BLOCK + threadIdx.x;
  if (p < w.np) lba_point_sum<FULL>(w, p);
}

// the tree: lane 0 ends with s[0] of the host's s[l] += s[l + stride]
__device__ inline double gba_tree(double v) {
#pragma unroll
  for (int stride = LBA_LANES / 2; stride >= 1; stride >>= 1) v = v + __shfl_down(v, stride);
  return v;
}

__global__ __launch_bounds__(LBA_LANES) void k_gba_pose(LbaWs w) {
  const int f = w.free_of_slot[blockIdx.x];
  double acc[27];
  lba_pose_lane(w, f, threadIdx.x, acc);
#pragma unroll
  for (int k = 0; k < 27; k++) acc[k] = gba_tree(acc[k]);
  if (threadIdx.x == 0) lba_pose_finish(w, f, acc);
}

__global__ __launch_bounds__(GBA_BLOCK) void k_gba_dinv(LbaWs w, double lambda) {
  const int p = blockIdx.x * GBA_BLOCK + threadIdx.x;
  if (p < w.np) lba_point_dinv(w, p, lambda);
}

__global__ __launch_bounds__(LBA_LANES) void k_gba_schur(GbaWs g, double lambda) {
  const int s1 = g.pair_s1[blockIdx.x], s2 = g.pair_s2[blockIdx.x];
  double acc[42];
  lba_schur_lane(g.l, g.l.free_of_slot[s1], g.l.free_of_slot[s2], threadIdx.x, acc);
#pragma unroll
  for (int k = 0; k < 42; k++) acc[k] = gba_tree(acc[k]);
  if (threadIdx.x == 0) gba_schur_finish(g, s1, s2, lambda, acc);
}

// Pivot block b: the diagonal block by thread 0, then the column below it. A trial that has failed
// (here, in an earlier pivot, or before the factorisation) leaves the envelope as it is.
__global__ __launch_bounds__(GBA_FACTOR_THREADS) void k_gba_pivot(GbaWs g, int b) {
  __shared__ double sD[36];
  __shared__ int s_fail;
  const int tid = threadIdx.x;
  if (tid == 0) {
    s_fail = g.l.rec->fail ? -1 : env_pivot_diag<6>(g.env, b, sD);
    if (s_fail > 0) lm_fail(g.l.rec, s_fail == 2 ? LM_FLAG_NONFINITE : 0u);
  }
  __syncthreads();
  if (s_fail) return;  // the same value in every thread
  const int rows = 6 * (g.env.col_begin[b + 1] - g.env.col_begin[b]);
  for (int t = tid; t < rows; t += GBA_FACTOR_THREADS) env_scale_row<6>(g.env, b, t, sD);
}

__global__ __launch_bounds__(GBA_FACTOR_THREADS) void k_gba_trailing(GbaWs g, int b) {
  if (g.l.rec->fail) return;
  const long long t = (long long)blockIdx.x * GBA_FACTOR_THREADS + threadIdx.x;
  if (t < env_trailing_items(g.env, b, 6)) env_trailing_item<6>(g.env, b, t);
}

// y holds the right-hand side throughout; xp is written only after a successful factorisation
__global__ __launch_bounds__(GBA_FACTOR_THREADS) void k_gba_subst(GbaWs g) {
  const EnvWs& e = g.env;
  const int tid = threadIdx.x, nt = GBA_FACTOR_THREADS, ns = e.ns, n = 6 * ns;
  __shared__ int s_fail;
  if (tid == 0) s_fail = g.l.rec->fail;
  __syncthreads();
  if (s_fail) return;
  for (int i = tid; i < n; i += nt) e.y[i] = g.l.bs[i];
  __syncthreads();
  for (int b = 0; b < ns; b++) {
    if (tid == 0) env_forward_diag<6>(e, b);
    __syncthreads();
    const int rows = 6 * (e.col_begin[b + 1] - e.col_begin[b]);
    for (int t = tid; t < rows; t += nt) env_forward_row<6>(e, b, t);
    __syncthreads();
  }
  for (int i = tid; i < n; i += nt) e.y[i] = e.y[i] / e.d[i];
  __syncthreads();
  for (int s = ns - 1; s >= 0; s--) {
    if (tid == 0) env_backward_diag<6>(e, s);
    __syncthreads();
    const int cols = 6 * (s - e.row_first[s]);
    for (int t = tid; t < cols; t += nt) env_backward_col<6>(e, s, t);
    __syncthreads();
  }
  for (int i = tid; i < n; i += nt) g.l.xp[i] = e.y[i];
}

__global__ __launch_bounds__(GBA_BLOCK) void k_gba_update(LbaWs w) {
  const int i = blockIdx.x * GBA_BLOCK + threadIdx.x;
  if (i < w.np) {
    if (!w.rec->fail) lba_point_backsub(w, i);  // after a failed solve x keeps its last values
    lba_update_point(w, i);
  } else if (i - w.np < w.nk) {
    lba_update_kf(w, i - w.np);
  }
}

__global__ __launch_bounds__(LBA_LANES) void k_gba_reduce(LbaWs w, int mode, double lambda) {
  double part[2];
  lba_reduce_lane(w, threadIdx.x, mode, lambda, part);
  const double chi = gba_tree(part[0]);
  double other;
  if (mode) {
    other = gba_tree(part[1]);
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

// ------------------------------------------------------------------------------------------
// host

struct orbfe_gba {
  int device = -1;
  int max_kf = 0, max_points = 0, max_edges = 0, max_env = 0;
  hipStream_t stream = nullptr;
  uint8_t* d_pool = nullptr;
  size_t pool_bytes = 0;
  LmRec* h_rec = nullptr;  // pinned
  GbaWs g;                  // device pointers, sized for the handle's bounds
};

static size_t gba_al(size_t b) { return (b + 255) & ~(size_t)255; }

// carves the device pool; with base == nullptr only the size is computed
static size_t gba_carve(orbfe_gba* h, uint8_t* base) {
  size_t off = 0;
  const size_t nk = h->max_kf, np = h->max_points, ne = h->max_edges, nb = h->max_env, n = 6 * nk;
  LbaWs& w = h->g.l;
  auto take = [&](size_t bytes) {
    uint8_t* p = base ? base + off : nullptr;
    off += gba_al(bytes);
    return p;
  };
#define GBA_TAKE(field, type, count) field = reinterpret_cast<type*>(take(sizeof(type) * (count)))
  GBA_TAKE(w.cam, const double, 5 * nk);
  GBA_TAKE(w.kf_free, const int, nk);
  GBA_TAKE(w.edge_begin, const int, np + 1);
  GBA_TAKE(w.e_kf, const int, ne);
  GBA_TAKE(w.e_pt, const int, ne);
  GBA_TAKE(w.e_obs, const double, 3 * ne);
  GBA_TAKE(w.e_w, const double, ne);
  GBA_TAKE(w.e_stereo, const uint8_t, ne);
  GBA_TAKE(w.kl_begin, const int, nk * LBA_LANES + 1);
  GBA_TAKE(w.kl_edge, const int, ne);
  GBA_TAKE(w.e_active, const uint8_t, ne);
  GBA_TAKE(w.p_active, const uint8_t, np);
  GBA_TAKE(w.slot_of_free, const int, nk);
  GBA_TAKE(w.free_of_slot, const int, nk);
  GBA_TAKE(w.est_T, double, 7 * nk);
  GBA_TAKE(w.tri_T, double, 7 * nk);
  GBA_TAKE(w.est_X, double, 3 * np);
  GBA_TAKE(w.tri_X, double, 3 * np);
  GBA_TAKE(w.e_err, double, 3 * ne);
  GBA_TAKE(w.e_prod, double, LBA_EDGE_DOUBLES * ne);
  GBA_TAKE(w.p_hll, double, 9 * np);
  GBA_TAKE(w.p_bl, double, 3 * np);
  GBA_TAKE(w.p_chi, double, np);
  GBA_TAKE(w.p_dinv, double, 9 * np);
  GBA_TAKE(w.p_db, double, 3 * np);
  GBA_TAKE(w.p_xl, double, 3 * np);
  GBA_TAKE(w.hpp, double, 21 * nk);
  GBA_TAKE(w.bp, double, 6 * nk);
  GBA_TAKE(w.bs, double, n);
  GBA_TAKE(w.d, double, n);
  GBA_TAKE(w.y, double, n);
  GBA_TAKE(w.xp, double, n);
  GBA_TAKE(w.rec, LmRec, 1);
  EnvWs& e = h->g.env;
  GBA_TAKE(e.row_first, const int, nk);
  GBA_TAKE(e.row_off, const int, nk + 1);
  GBA_TAKE(e.col_begin, const int, nk + 1);
  GBA_TAKE(e.col_row, const int, nb);
  GBA_TAKE(e.L, double, 36 * nb);
  GBA_TAKE(h->g.pair_s1, const int, nb);
  GBA_TAKE(h->g.pair_s2, const int, nb);
#undef GBA_TAKE
  e.d = w.d, e.y = w.y;
  return off;
}

extern "C" int orbfe_gba_create(int device, int max_kf, int max_points, int max_edges, int max_env_blocks, orbfe_gba** out) {
  if (!out) return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_gba_create: bad argument");
  *out = nullptr;
  if (max_kf < 1 || max_kf > ORBFE_GBA_MAX_KF || max_points < 1 || max_points > ORBFE_GBA_MAX_POINTS || max_edges < 1 ||
      max_edges > ORBFE_GBA_MAX_EDGES || max_env_blocks < 1 || max_env_blocks > ORBFE_GBA_MAX_ENV_BLOCKS)
    return orbfe_set_error(ORBFE_ERR_ARG,
                           "orbfe_gba_create: max_kf in 1..4096, max_points in 1..524288, max_edges in 1..4194304, "
                           "max_env_blocks in 1..2097152");
  orbfe_gba* h = new orbfe_gba();
  memset(&h->g, 0, sizeof(h->g));
  h->max_kf = max_kf, h->max_points = max_points, h->max_edges = max_edges, h->max_env = max_env_blocks;
  if (device < 0) {
    *out = h;
    return ORBFE_OK;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device >= ndev) {
    delete h;
    return orbfe_set_error(ORBFE_ERR_HIP, "orbfe_gba_create: no such HIP device");
  }
  h->device = device;
  h->pool_bytes = gba_carve(h, nullptr);
  auto fail = [&](hipError_t e, const char* what) {
    const int st = orbfe_set_hip_error(e, what);
    orbfe_gba_destroy(h);
    return st;
  };
#define GBA_TRY(expr)                             \
  do {                                            \
    hipError_t _e = (expr);                       \
    if (_e != hipSuccess) return fail(_e, #expr); \
  } while (0)
  GBA_TRY(hipSetDevice(device));
  GBA_TRY(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  GBA_TRY(hipMalloc(&h->d_pool, h->pool_bytes));
  GBA_TRY(hipHostMalloc(&h->h_rec, sizeof(LmRec), hipHostMallocDefault));
#undef GBA_TRY
  gba_carve(h, h->d_pool);
  *out = h;
  return ORBFE_OK;
}

extern "C" int orbfe_gba_destroy(orbfe_gba* h) {
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
inline unsigned gba_grid(long long n, int block) { return (unsigned)((n + block - 1) / block); }

// gba_run's backend over the handle's device workspace
struct GbaDevBackend {
  orbfe_gba* h;
  GbaWs g;
  const GbaEnvPlan* E;

  template <class T>
  int up(const T* dst, const T* src, size_t count) {
    if (count == 0) return ORBFE_OK;
    ORBFE_HIP_CHECK(hipMemcpyAsync(const_cast<T*>(dst), src, sizeof(T) * count, hipMemcpyHostToDevice, h->stream));
    ORBFE_HIP_CHECK(hipStreamSynchronize(h->stream));  // the source may be pageable and short-lived
    return ORBFE_OK;
  }

  int start(const LbaPlan& P, const GbaEnvPlan& env) {
    g = h->g;
    E = &env;
    LbaWs& w = g.l;
    w.nk = P.nk, w.nfree = P.nfree, w.np = P.np, w.ne = P.ne, w.nslot = 0, w.kernel_on = 1;
    gba_set_deltas(&w);
    g.env.ns = env.ns, g.npair = (int)env.npair;
    int st;
#define GBA_UP(dst, src, count) \
  if ((st = up(dst, src, count)) != ORBFE_OK) return st
    GBA_UP(w.cam, P.cam.data(), P.cam.size());
    GBA_UP(w.kf_free, P.kf_free.data(), P.kf_free.size());
    GBA_UP(w.edge_begin, P.edge_begin, (size_t)P.np + 1);
    GBA_UP(w.e_kf, P.e_kf, (size_t)P.ne);
    GBA_UP(w.e_pt, P.e_pt.data(), P.e_pt.size());
    GBA_UP(w.e_obs, P.e_obs.data(), P.e_obs.size());
    GBA_UP(w.e_w, P.e_w.data(), P.e_w.size());
    GBA_UP(w.e_stereo, P.e_stereo.data(), P.e_stereo.size());
    GBA_UP(w.kl_begin, P.kl_begin.data(), P.kl_begin.size());
    GBA_UP(w.kl_edge, P.kl_edge.data(), P.kl_edge.size());
    GBA_UP((const double*)w.est_T, P.T0.data(), P.T0.size());
    GBA_UP((const double*)w.tri_T, P.T0.data(), P.T0.size());
    GBA_UP((const double*)w.est_X, P.X0.data(), P.X0.size());
    GBA_UP((const double*)w.tri_X, P.X0.data(), P.X0.size());
    GBA_UP(g.env.row_first, env.row_first.data(), env.row_first.size());
    GBA_UP(g.env.row_off, env.row_off.data(), env.row_off.size());
    GBA_UP(g.env.col_begin, env.col_begin.data(), env.col_begin.size());
    GBA_UP(g.env.col_row, env.col_row.data(), env.col_row.size());
    GBA_UP(g.pair_s1, env.pair_s1.data(), env.pair_s1.size());
    GBA_UP(g.pair_s2, env.pair_s2.data(), env.pair_s2.size());
    ORBFE_HIP_CHECK(hipMemsetAsync(w.e_err, 0, sizeof(double) * 3 * (size_t)P.ne, h->stream));
    return ORBFE_OK;
  }

  int begin_round(const LbaActive& A, bool kernel_on) {
    int st;
    LbaWs& w = g.l;
    GBA_UP(w.e_active, A.e_active.data(), A.e_active.size());
    GBA_UP(w.p_active, A.p_active.data(), A.p_active.size());
    GBA_UP(w.slot_of_free, A.slot_of_free.data(), A.slot_of_free.size());
    GBA_UP(w.free_of_slot, A.free_of_slot.data(), A.free_of_slot.size());
#undef GBA_UP
    w.nslot = A.nslot, w.kernel_on = kernel_on ? 1 : 0;
    if (w.nslot > 0) ORBFE_HIP_CHECK(hipMemsetAsync(w.xp, 0, sizeof(double) * 6 * (size_t)w.nslot, h->stream));
    ORBFE_HIP_CHECK(hipMemsetAsync(w.p_xl, 0, sizeof(double) * 3 * (size_t)w.np, h->stream));
    return ORBFE_OK;
  }

  int read_rec(LmRec* out) {
    ORBFE_HIP_CHECK(hipGetLastError());
    ORBFE_HIP_CHECK(hipMemcpyAsync(h->h_rec, g.l.rec, sizeof(LmRec), hipMemcpyDeviceToHost, h->stream));
    ORBFE_HIP_CHECK(hipStreamSynchronize(h->stream));
    *out = *h->h_rec;
    return ORBFE_OK;
  }

  int linearize(LmRec* out) {
    const LbaWs& w = g.l;
    ORBFE_HIP_CHECK(hipMemsetAsync(w.rec, 0, sizeof(LmRec), h->stream));
    ORBFE_LAUNCH("k_gba_edge", k_gba_edge<true>, dim3(gba_grid(w.ne, GBA_BLOCK)), dim3(GBA_BLOCK), 0, h->stream, w, 0);
    ORBFE_LAUNCH("k_gba_point", k_gba_point<true>, dim3(gba_grid(w.np, GBA_BLOCK)), dim3(GBA_BLOCK), 0, h->stream, w);
    if (w.nslot > 0) ORBFE_LAUNCH("k_gba_pose", k_gba_pose, dim3(w.nslot), dim3(LBA_LANES), 0, h->stream, w);
    ORBFE_LAUNCH("k_gba_reduce", k_gba_reduce, dim3(1), dim3(LBA_LANES), 0, h->stream, w, 0, 0.0);
    return read_rec(out);
  }

  int trial(double lambda, LmRec* out) {
    const LbaWs& w = g.l;
    ORBFE_HIP_CHECK(hipMemsetAsync(w.rec, 0, sizeof(LmRec), h->stream));
    ORBFE_LAUNCH("k_gba_dinv", k_gba_dinv, dim3(gba_grid(w.np, GBA_BLOCK)), dim3(GBA_BLOCK), 0, h->stream, w, lambda);
    if (g.env.ns > 0) {
      // blocks without a structural pair are +0.0 before the factorisation
      ORBFE_HIP_CHECK(hipMemsetAsync(g.env.L, 0, sizeof(double) * 36 * (size_t)E->nblk, h->stream));
      ORBFE_LAUNCH("k_gba_schur", k_gba_schur, dim3(g.npair), dim3(LBA_LANES), 0, h->stream, g, lambda);
      for (int b = 0; b < g.env.ns; b++) {
        ORBFE_LAUNCH("k_gba_pivot", k_gba_pivot, dim3(1), dim3(GBA_FACTOR_THREADS), 0, h->stream, g, b);
        const long long nr = E->col_begin[b + 1] - E->col_begin[b];
        if (nr > 0)
          ORBFE_LAUNCH("k_gba_trailing", k_gba_trailing, dim3(gba_grid(nr * nr * 36, GBA_FACTOR_THREADS)), dim3(GBA_FACTOR_THREADS), 0,
                       h->stream, g, b);
      }
      ORBFE_LAUNCH("k_gba_subst", k_gba_subst, dim3(1), dim3(GBA_FACTOR_THREADS), 0, h->stream, g);
    }
    ORBFE_LAUNCH("k_gba_update", k_gba_update, dim3(gba_grid((long long)w.np + w.nk, GBA_BLOCK)), dim3(GBA_BLOCK), 0, h->stream, w);
    ORBFE_LAUNCH("k_gba_edge_trial", k_gba_edge<false>, dim3(gba_grid(w.ne, GBA_BLOCK)), dim3(GBA_BLOCK), 0, h->stream, w, 1);
    ORBFE_LAUNCH("k_gba_point_chi", k_gba_point<false>, dim3(gba_grid(w.np, GBA_BLOCK)), dim3(GBA_BLOCK), 0, h->stream, w);
    ORBFE_LAUNCH("k_gba_reduce", k_gba_reduce, dim3(1), dim3(LBA_LANES), 0, h->stream, w, 1, lambda);
    return read_rec(out);
  }

  int accept() {  // discardTop: the trial estimates become the accepted ones
    LbaWs& w = g.l;
    double* t = w.est_T;
    w.est_T = w.tri_T, w.tri_T = t;
    t = w.est_X;
    w.est_X = w.tri_X, w.tri_X = t;
    return ORBFE_OK;
  }

  int finish(double* T, double* X) {
    const LbaWs& w = g.l;
    ORBFE_HIP_CHECK(hipMemcpyAsync(T, w.est_T, sizeof(double) * 7 * (size_t)w.nk, hipMemcpyDeviceToHost, h->stream));
    ORBFE_HIP_CHECK(hipMemcpyAsync(X, w.est_X, sizeof(double) * 3 * (size_t)w.np, hipMemcpyDeviceToHost, h->stream));
    ORBFE_HIP_CHECK(hipStreamSynchronize(h->stream));
    return ORBFE_OK;
  }
};

// the boundary: everything a kernel will use as an index. r may be null (orbfe_gba_envelope).
int gba_check(const char* who, int max_kf, int max_points, int max_edges, const orbfe_gba_problem_t* p, const orbfe_gba_result_t* r) {
  char msg[160];
  auto err = [&](int st, const char* what) {
    snprintf(msg, sizeof(msg), "%s: %s", who, what);
    return orbfe_set_error(st, msg);
  };
  if (p->n_kf < 0 || p->n_points < 0 || p->n_edges < 0) return err(ORBFE_ERR_ARG, "negative count");
  if (p->n_kf > max_kf || p->n_points > max_points || p->n_edges > max_edges) return err(ORBFE_ERR_CAPACITY, "problem above the bounds");
  if (!p->edge_begin || (p->n_kf > 0 && (!p->tcw || !p->k || !p->bf || !p->fixed || (r && !r->tcw))) ||
      (p->n_points > 0 && (!p->xw || (r && !r->xw))) || (p->n_edges > 0 && (!p->edge_kf || !p->kp_un || !p->u_right || !p->inv_sigma2)))
    return err(ORBFE_ERR_ARG, "null array");
  if (p->n_iterations < 1 || p->n_iterations > ORBFE_GBA_MAX_ITERATIONS) return err(ORBFE_ERR_ARG, "n_iterations outside 1..64");
  if (p->stop_at_poll < -1) return err(ORBFE_ERR_ARG, "stop_at_poll below -1");
  if (p->edge_begin[0] != 0 || p->edge_begin[p->n_points] != p->n_edges) return err(ORBFE_ERR_ARG, "edge_begin is not a CSR over n_edges");
  std::vector<int> seen(p->n_kf > 0 ? p->n_kf : 1, -1);
  for (int q = 0; q < p->n_points; q++) {
    const int b = p->edge_begin[q], e = p->edge_begin[q + 1];
    if (b > e || b < 0 || e > p->n_edges) return err(ORBFE_ERR_ARG, "edge_begin is not a CSR over n_edges");
    for (int i = b; i < e; i++) {
      const int kf = p->edge_kf[i];
      if (kf < 0 || kf >= p->n_kf) return err(ORBFE_ERR_ARG, "keyframe index out of range");
      if (seen[kf] == q) return err(ORBFE_ERR_ARG, "a keyframe listed twice under one point");
      seen[kf] = q;
    }
  }
  return ORBFE_OK;
}

struct GbaPlans {
  GbaIn in;
  LbaPlan plan;
  LbaActive A;
  GbaEnvPlan E;
};

void gba_plans(const orbfe_gba_problem_t* p, long long max_blocks, GbaPlans* o) {
  o->in = {{p->n_kf, p->n_points, p->n_edges, p->tcw, p->k, p->bf, p->fixed, p->xw, p->edge_begin, p->edge_kf, p->kp_un, p->u_right,
            p->inv_sigma2, p->stop_flag, p->stop_at_poll},
           p->n_iterations,
           p->robust};
  lba_plan(o->in.l, &o->plan);
  lba_active(o->in.l, o->plan, nullptr, &o->A);
  gba_plan_envelope(o->in.l, o->plan, o->A, max_blocks, &o->E);
}
}  // namespace

extern "C" int orbfe_gba_envelope(const orbfe_gba_problem_t* p, int* env_blocks, int* schur_blocks) {
  if (!p || !env_blocks || !schur_blocks) return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_gba_envelope: bad argument");
  int st = gba_check("orbfe_gba_envelope", ORBFE_GBA_MAX_KF, ORBFE_GBA_MAX_POINTS, ORBFE_GBA_MAX_EDGES, p, nullptr);
  if (st != ORBFE_OK) return st;
  GbaPlans pl;
  gba_plans(p, ORBFE_GBA_MAX_ENV_BLOCKS, &pl);
  if (pl.E.nblk > ORBFE_GBA_MAX_ENV_BLOCKS) return orbfe_set_error(ORBFE_ERR_CAPACITY, "orbfe_gba_envelope: envelope above 2097152 blocks");
  *env_blocks = (int)pl.E.nblk, *schur_blocks = (int)pl.E.npair;
  return ORBFE_OK;
}

extern "C" int orbfe_gba_solve(orbfe_gba* h, const orbfe_gba_problem_t* p, orbfe_gba_result_t* r) {
  if (!h || !p || !r) return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_gba_solve: bad argument");
  int st = gba_check("orbfe_gba_solve", h->max_kf, h->max_points, h->max_edges, p, r);
  if (st != ORBFE_OK) return st;
  GbaPlans pl;
  gba_plans(p, h->max_env, &pl);
  if (pl.E.nblk > h->max_env) return orbfe_set_error(ORBFE_ERR_CAPACITY, "orbfe_gba_solve: envelope above the handle's max_env_blocks");
  if (h->device < 0) return orbfe_set_error(ORBFE_ERR_STATE, "global bundle adjuster is host-only (device < 0)");
  GbaOut o;
  ORBFE_HIP_CHECK(hipSetDevice(h->device));
  GbaDevBackend b = {h, h->g, nullptr};
  st = gba_run(b, pl.in, pl.plan, pl.A, pl.E, &o);
  if (st != ORBFE_OK) return st;
  if (p->n_kf > 0) memcpy(r->tcw, o.tcw.data(), sizeof(float) * o.tcw.size());
  if (p->n_points > 0) memcpy(r->xw, o.xw.data(), sizeof(float) * o.xw.size());
  memcpy(&r->trace, &o.trace, sizeof(r->trace));
  return ORBFE_OK;
}
