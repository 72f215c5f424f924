// orbfe_gba.hip -- Optimizer::BundleAdjustment on the GPU (include/orbfe_gba.h): a whole map's
// Levenberg-Marquardt, the Schur complement over the covisible keyframe pairs, the reduced system a 6x6
// block envelope factorised across workgroups.
//
// The Levenberg control flow (gba_run of orbfe_gba_core.h over lm_host_optimize) runs on the host and
// reads one LmRec per linearisation and per trial; the stages are kernels on the handle's one stream:
//   k_gba_edge / point / pose / dinv / update / reduce   orbfe_ba_device.h's k_ba_* kernels, the one set
//                   orbfe_lba.hip launches too, under this file's labels for the kernel timer
//   k_gba_schur     one wavefront per structural pair: the Schur block into the envelope's lower triangle
//                   and, on the diagonal pairs, bschur
//   k_gba_pivot     per pivot block, one workgroup: the 6x6 diagonal factorisation, then the column below
//                   it scaled, one scalar row per thread
//   k_gba_trailing  per pivot block, grid-wide: one thread per scalar of one (a, bb) block of the column's
//                   rows, its six updates in ascending p
//   k_gba_subst     one workgroup: the forward and the backward substitution over the envelope
// k_gba_pivot, k_gba_trailing and k_gba_subst run orbfe_env_core.h's routines at block dimension 6; they
// are orbfe_essgraph.hip's k_eg_factor (the same routines at 7) split at its __syncthreads() boundaries. No
// kernel waits on another workgroup: the stream orders them, about 2 n_slots launches per trial. Every index a kernel reads was checked by orbfe_gba_solve or built by lba_plan / lba_active /
// gba_plan_envelope; every loop runs to a count among those.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>
#include <vector>

#include "../../include/orbfe_gba.h"
#include "orbfe_ba_device.h"
#include "orbfe_gba_core.h"

static_assert(LM_FLAG_LARGE_STEP == ORBFE_GBA_FLAG_LARGE_STEP && LM_FLAG_NONFINITE == ORBFE_GBA_FLAG_NONFINITE, "flag values");
static_assert(LM_STOP_ALL == ORBFE_GBA_STOP_ALL && LM_STOP_TERMINATE == ORBFE_GBA_STOP_TERMINATE &&
                  LM_STOP_NBAD == ORBFE_GBA_STOP_NBAD && LM_STOP_NO_EDGE == ORBFE_GBA_STOP_NO_EDGE &&
                  LM_STOP_FLAG == ORBFE_GBA_STOP_FLAG,
              "stop codes");
static_assert(sizeof(GbaTrace) == sizeof(orbfe_gba_trace_t), "trace layout");

#define GBA_FACTOR_THREADS 256

__global__ __launch_bounds__(LBA_LANES) void k_gba_schur(GbaWs g, double lambda) {
  const int s1 = g.pair_s1[blockIdx.x], s2 = g.pair_s2[blockIdx.x];
  double acc[42];
  lba_schur_lane(g.l, g.l.free_of_slot[s1], g.l.free_of_slot[s2], threadIdx.x, acc);
#pragma unroll
  for (int k = 0; k < 42; k++) acc[k] = ba_tree(acc[k]);
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
  for (int t = tid; t < rows; t += GBA_FACTOR_THREADS) env_scale_row<6>(g.env, b, t, sD, g.env.d + 6 * b);
}

__global__ __launch_bounds__(GBA_FACTOR_THREADS) void k_gba_trailing(GbaWs g, int b) {
  if (g.l.rec->fail) return;
  const long long t = (long long)blockIdx.x * GBA_FACTOR_THREADS + threadIdx.x;
  if (t < env_trailing_items(g.env, b, 6)) env_trailing_item<6>(g.env, b, t, g.env.d + 6 * b);
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

// ------------------------------------------------------------------------------------------
// host

struct orbfe_gba : OrbfeDev {
  int max_kf = 0, max_points = 0, max_edges = 0, max_env = 0;
  uint8_t* d_pool = nullptr;
  size_t pool_bytes = 0;
  LmRec* h_rec = nullptr;  // pinned
  GbaWs g;                  // device pointers, sized for the handle's bounds
};

// carves the device pool; with base == nullptr only the size is computed
static size_t gba_carve(orbfe_gba* h, uint8_t* base) {
  const size_t nk = h->max_kf, nb = h->max_env;
  OrbfeStage pool;
  pool.d = base;
  ba_carve(pool, h->g.l, nk, nk, h->max_points, h->max_edges, false);
  EnvWs& e = h->g.env;
  pool.take(e.row_first, nk);
  pool.take(e.row_off, nk + 1);
  pool.take(e.col_begin, nk + 1);
  pool.take(e.col_row, nb);
  pool.take(e.L, 36 * nb);
  pool.take(h->g.pair_s1, nb);
  pool.take(h->g.pair_s2, nb);
  e.d = h->g.l.d, e.y = h->g.l.y;
  return pool.off;
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
  const int open_st = orbfe_dev_open(h, device, "orbfe_gba_create");
  if (open_st != ORBFE_OK) {
    orbfe_gba_destroy(h);
    return open_st;
  }
  h->pool_bytes = gba_carve(h, nullptr);
  ORBFE_CREATE_HIP(h, orbfe_gba_destroy, hipMalloc(&h->d_pool, h->pool_bytes));
  ORBFE_CREATE_HIP(h, orbfe_gba_destroy, hipHostMalloc(&h->h_rec, sizeof(LmRec), hipHostMallocDefault));
  gba_carve(h, h->d_pool);
  *out = h;
  return ORBFE_OK;
}

extern "C" int orbfe_gba_destroy(orbfe_gba* h) {
  if (!h) return ORBFE_OK;
  if (orbfe_dev_close(h)) {
    hipFree(h->d_pool);
    if (h->h_rec) hipHostFree(h->h_rec);
  }
  delete h;
  return ORBFE_OK;
}

namespace {
const BaNames kGbaNames = {"k_gba_edge",   "k_gba_point",      "k_gba_pose",      "k_gba_dinv",
                           "k_gba_update", "k_gba_edge_trial", "k_gba_point_chi", "k_gba_reduce"};

// gba_run's backend: BaDevBackend with the envelope as the reduced system
struct GbaDevBackend : BaDevBackend {
  orbfe_gba* h;
  GbaWs g;  // g.l is a copy of w, taken per trial
  const GbaEnvPlan* E;

  int start(const LbaPlan& P, const GbaEnvPlan& env) {
    w = h->g.l, g = h->g;
    E = &env;
    gba_set_deltas(&w);
    g.env.ns = env.ns, g.npair = (int)env.npair;
    int st = BaDevBackend::start(P);
    if (st != ORBFE_OK) return st;
    BA_UP(g.env.row_first, env.row_first.data(), env.row_first.size());
    BA_UP(g.env.row_off, env.row_off.data(), env.row_off.size());
    BA_UP(g.env.col_begin, env.col_begin.data(), env.col_begin.size());
    BA_UP(g.env.col_row, env.col_row.data(), env.col_row.size());
    BA_UP(g.pair_s1, env.pair_s1.data(), env.pair_s1.size());
    BA_UP(g.pair_s2, env.pair_s2.data(), env.pair_s2.size());
    return ORBFE_OK;
  }

  int begin_round(const LbaActive& A, bool kernel_on) { return BaDevBackend::begin_round(A, kernel_on, 6 * (size_t)A.nslot); }

  int trial(double lambda, LmRec* out) {
    int st = begin_trial(lambda);
    if (st != ORBFE_OK) return st;
    g.l = w;
    if (g.env.ns > 0) {
      // blocks without a structural pair are +0.0 before the factorisation
      ORBFE_HIP_CHECK(hipMemsetAsync(g.env.L, 0, sizeof(double) * 36 * (size_t)E->nblk, stream));
      ORBFE_LAUNCH("k_gba_schur", k_gba_schur, dim3(g.npair), dim3(LBA_LANES), 0, stream, g, lambda);
      for (int b = 0; b < g.env.ns; b++) {
        ORBFE_LAUNCH("k_gba_pivot", k_gba_pivot, dim3(1), dim3(GBA_FACTOR_THREADS), 0, stream, g, b);
        const long long nr = E->col_begin[b + 1] - E->col_begin[b];
        if (nr > 0)
          ORBFE_LAUNCH("k_gba_trailing", k_gba_trailing, dim3(ba_grid(nr * nr * 36, GBA_FACTOR_THREADS)), dim3(GBA_FACTOR_THREADS), 0,
                       stream, g, b);
      }
      ORBFE_LAUNCH("k_gba_subst", k_gba_subst, dim3(1), dim3(GBA_FACTOR_THREADS), 0, stream, g);
    }
    return end_trial(lambda, out);
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
  return ba_check_csr(who, p->n_kf, p->n_points, p->n_edges, p->edge_begin, p->edge_kf);
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
  GbaDevBackend b = {{h->stream, h->h_rec, h->g.l, &kGbaNames}, h, h->g, nullptr};
  st = gba_run(b, pl.in, pl.plan, pl.A, pl.E, &o);
  if (st != ORBFE_OK) return st;
  if (p->n_kf > 0) memcpy(r->tcw, o.tcw.data(), sizeof(float) * o.tcw.size());
  if (p->n_points > 0) memcpy(r->xw, o.xw.data(), sizeof(float) * o.xw.size());
  memcpy(&r->trace, &o.trace, sizeof(r->trace));
  return ORBFE_OK;
}
