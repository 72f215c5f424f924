// orbfe_essgraph.hip -- Optimizer::OptimizeEssentialGraph on the GPU (include/orbfe_essgraph.h): the
// pose-graph Levenberg-Marquardt over Sim3 vertices with a sparse LDL^T over the block envelope.
//
// The Levenberg control flow (eg_run of orbfe_essgraph_core.h over lm_host_optimize of orbfe_lm_core.h) runs
// on the host and reads one LmRec per linearisation and per trial; the stages are kernels on the handle's
// one stream, each a thread- or lane-per-element call of the core header's functions:
//   k_eg_vertex_setup  per vertex: vScw, the start estimate, the measurement-side state
//   k_eg_edge_setup    per edge: the measurement
//   k_eg_linearize     32 lanes per edge: the 29 error evaluations one per lane, the 7 x 14 Jacobian in
//                      LDS, the edge's 161 products
//   k_eg_assemble      64 lanes per block: a diagonal block with b_s, or an off-diagonal block that has
//                      edges, summed in ascending edge index
//   k_eg_lambda        per diagonal scalar: + lambda on the copy
//   k_eg_factor        one workgroup: orbfe_env_core.h's block LDL^T over the envelope (per pivot block:
//                      its 7 x 7 factorisation, the scaled column below, the trailing updates), then the
//                      forward and the backward substitution; the routines orbfe_gba.hip runs as
//                      k_gba_pivot / trailing / subst
//   k_eg_update        per vertex: oplus into the trial estimate
//   k_eg_chi           per edge: the error at the trial estimates
//   k_eg_reduce        one wavefront: the total chi2 and computeScale by the 64-lane rule
//   k_eg_finish        per vertex: [R | t / s]; per point: the two maps
// No kernel waits on another: the stream orders them. Every index a kernel reads was checked by
// orbfe_essgraph_solve or built by eg_plan; every loop runs to a count among those.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>
#include <vector>

#include "../../include/orbfe_essgraph.h"
#include "orbfe_device.h"
#include "orbfe_essgraph_core.h"
#include "orbfe_ktimer.h"
#include "orbfe_stage.h"

static_assert(LM_FLAG_LARGE_STEP == ORBFE_ESSGRAPH_FLAG_LARGE_STEP && LM_FLAG_NONFINITE == ORBFE_ESSGRAPH_FLAG_NONFINITE,
              "flag values");
static_assert(LM_STOP_ALL == ORBFE_ESSGRAPH_STOP_ALL && LM_STOP_TERMINATE == ORBFE_ESSGRAPH_STOP_TERMINATE &&
                  LM_STOP_NBAD == ORBFE_ESSGRAPH_STOP_NBAD && LM_STOP_NO_EDGE == ORBFE_ESSGRAPH_STOP_NO_EDGE,
              "stop codes");
static_assert(sizeof(EgTrace) == sizeof(orbfe_essgraph_trace_t), "trace layout");

#define EG_BLOCK 128
#define EG_LIN_LANES 32  // lanes per edge in k_eg_linearize
#define EG_LIN_EDGES 4   // edges per workgroup
#define EG_FACTOR_THREADS 1024
static_assert(EG_STATES <= EG_LIN_LANES, "one state per lane");

__global__ __launch_bounds__(EG_BLOCK) void k_eg_vertex_setup(EgWs w) {
  const int v = blockIdx.x * EG_BLOCK + threadIdx.x;
  if (v < w.nv) eg_vertex_setup(w, v);
}

__global__ __launch_bounds__(EG_BLOCK) void k_eg_edge_setup(EgWs w) {
  const int e = blockIdx.x * EG_BLOCK + threadIdx.x;
  if (e < w.ne) eg_edge_setup(w, e);
}

__global__ __launch_bounds__(EG_LIN_LANES* EG_LIN_EDGES) void k_eg_linearize(EgWs w) {
  __shared__ double sJ[EG_LIN_EDGES][98];
  const int g = threadIdx.x / EG_LIN_LANES, lane = threadIdx.x % EG_LIN_LANES;
  const int e = blockIdx.x * EG_LIN_EDGES + g;
  const bool on = e < w.ne;
  if (on && lane < EG_STATES) eg_edge_state(w, e, lane, w.est);
  __syncthreads();  // the group's 29 errors are in e_state
  const double* st = w.e_state + (size_t)(on ? e : 0) * EG_STATES * 7;
  if (on)
    for (int t = lane; t < 98; t += EG_LIN_LANES) sJ[g][t] = eg_jac(st, t / 14, t % 14);
  __syncthreads();
  if (on)
    for (int idx = lane; idx < EG_EDGE_DOUBLES; idx += EG_LIN_LANES)
      w.e_prod[EG_EDGE_DOUBLES * (size_t)e + idx] = eg_product(sJ[g], st, idx);
}

__global__ __launch_bounds__(EG_LANES) void k_eg_assemble(EgWs w) {
  const int item = blockIdx.x, idx = threadIdx.x;
  if (item < w.ns) {
    if (idx < 56) eg_diag_entry(w, item, idx);
  } else if (idx < 49) {
    eg_offdiag_entry(w, item - w.ns, idx);
  }
}

__global__ __launch_bounds__(EG_BLOCK) void k_eg_lambda(EgWs w, double lambda) {
  const int t = blockIdx.x * EG_BLOCK + threadIdx.x;
  if (t < 7 * w.ns) eg_add_lambda(w, t / 7, t % 7, lambda);
}

// orbfe_env_core.h's factorisation and substitutions (env_*<7>) by one workgroup: per pivot block its
// diagonal block by thread 0, the column below it one scalar row per thread, the trailing updates one
// scalar per thread; then the forward and the backward substitution, block by block. y holds the
// right-hand side throughout; x is written only after a successful factorisation.
__global__ __launch_bounds__(EG_FACTOR_THREADS) void k_eg_factor(EgWs w) {
  __shared__ double sD[49];
  __shared__ double sd[7];  // the pivot block's d: the bits of e.d, read by every thread of the two loops below
  __shared__ int s_fail;
  const EnvWs e = eg_env(w);
  const int tid = threadIdx.x, nt = EG_FACTOR_THREADS, ns = e.ns, n = 7 * ns;
  for (int b = 0; b < ns; b++) {
    if (tid == 0) {
      s_fail = env_pivot_diag<7>(e, b, sD);
      for (int p = 0; p < 7; p++) sd[p] = sD[8 * p];
    }
    __syncthreads();
    if (s_fail) {  // the same value in every thread
      if (tid == 0) lm_fail(w.rec, s_fail == 2 ? LM_FLAG_NONFINITE : 0u);
      return;
    }
    const int rows = 7 * (e.col_begin[b + 1] - e.col_begin[b]);
    for (int t = tid; t < rows; t += nt) env_scale_row<7>(e, b, t, sD, sd);
    __syncthreads();
    const long long items = env_trailing_items(e, b, 7);
    for (long long t = tid; t < items; t += nt) env_trailing_item<7>(e, b, t, sd);
    __syncthreads();
  }
  for (int i = tid; i < n; i += nt) e.y[i] = w.b[i];
  __syncthreads();
  for (int b = 0; b < ns; b++) {
    if (tid == 0) env_forward_diag<7>(e, b);
    __syncthreads();
    const int rows = 7 * (e.col_begin[b + 1] - e.col_begin[b]);
    for (int t = tid; t < rows; t += nt) env_forward_row<7>(e, b, t);
    __syncthreads();
  }
  for (int i = tid; i < n; i += nt) e.y[i] = e.y[i] / e.d[i];
  __syncthreads();
  for (int s = ns - 1; s >= 0; s--) {
    if (tid == 0) env_backward_diag<7>(e, s);
    __syncthreads();
    const int cols = 7 * (s - e.row_first[s]);
    for (int t = tid; t < cols; t += nt) env_backward_col<7>(e, s, t);
    __syncthreads();
  }
  for (int i = tid; i < n; i += nt) w.x[i] = e.y[i];
}

__global__ __launch_bounds__(EG_BLOCK) void k_eg_update(EgWs w) {
  const int v = blockIdx.x * EG_BLOCK + threadIdx.x;
  if (v < w.nv) eg_update_vertex(w, v);
}

__global__ __launch_bounds__(EG_BLOCK) void k_eg_chi(EgWs w) {
  const int e = blockIdx.x * EG_BLOCK + threadIdx.x;
  if (e < w.ne) eg_edge_chi(w, e, w.tri);
}

__global__ __launch_bounds__(EG_LANES) void k_eg_reduce(EgWs w, int mode, double lambda) {
  double part[2];
  eg_reduce_lane(w, threadIdx.x, mode, lambda, part);
#pragma unroll
  for (int stride = EG_LANES / 2; stride >= 1; stride >>= 1) {
    part[0] = part[0] + __shfl_down(part[0], stride);
    part[1] = part[1] + __shfl_down(part[1], stride);
  }
  if (threadIdx.x == 0) w.rec->chi = part[0], w.rec->scale = part[1];
}

__global__ __launch_bounds__(EG_BLOCK) void k_eg_finish(EgWs w) {
  const size_t i = (size_t)blockIdx.x * EG_BLOCK + threadIdx.x;
  if (i < (size_t)w.np) eg_finish_point(w, (int)i);
  else if (i - w.np < (size_t)w.nv) eg_finish_vertex(w, (int)(i - w.np));
}

// ------------------------------------------------------------------------------------------
// host

struct orbfe_essgraph : OrbfeDev {
  int max_v = 0, max_e = 0, max_blk = 0, max_p = 0;
  uint8_t* d_pool = nullptr;
  size_t pool_bytes = 0;
  LmRec* h_rec = nullptr;  // pinned
  EgWs w;                  // device pointers, sized for the handle's bounds
};

// carves the device pool; with base == nullptr only the size is computed
static size_t eg_carve(orbfe_essgraph* h, uint8_t* base) {
  OrbfeStage pool;
  pool.d = base;
  const size_t nv = h->max_v, ne = h->max_e, nb = h->max_blk, np = h->max_p;
  EgWs& w = h->w;
  pool.take(w.tcw, 12 * nv);
  pool.take(w.corr_of_v, nv);
  pool.take(w.nonc_of_v, nv);
  pool.take(w.corr, 8 * nv);
  pool.take(w.nonc, 8 * nv);
  pool.take(w.e_i, ne);
  pool.take(w.e_j, ne);
  pool.take(w.e_kind, ne);
  pool.take(w.xw, 3 * np);
  pool.take(w.p_ref, np);
  pool.take(w.slot_of_v, nv);
  pool.take(w.v_of_slot, nv);
  pool.take(w.ve_begin, nv + 1);
  pool.take(w.ve_edge, 2 * ne);
  pool.take(w.row_first, nv);
  pool.take(w.row_off, nv + 1);
  pool.take(w.ob_begin, ne + 1);
  pool.take(w.ob_pos, ne);
  pool.take(w.ob_edge, ne);
  pool.take(w.col_begin, nv + 1);
  pool.take(w.col_row, nb);
  pool.take(w.scw, 8 * nv);
  pool.take(w.mst, 8 * nv);
  pool.take(w.est, 8 * nv);
  pool.take(w.tri, 8 * nv);
  pool.take(w.meas, 8 * ne);
  pool.take(w.e_state, EG_STATES * 7 * ne);
  pool.take(w.e_chi, ne);
  pool.take(w.e_prod, EG_EDGE_DOUBLES * ne);
  pool.take(w.H, 49 * nb);
  pool.take(w.L, 49 * nb);
  pool.take(w.b, 7 * nv);
  pool.take(w.d, 7 * nv);
  pool.take(w.y, 7 * nv);
  pool.take(w.x, 7 * nv);
  pool.take(w.out_tcw, 12 * nv);
  pool.take(w.out_xw, 3 * np);
  pool.take(w.rec, 1);
  return pool.off;
}

extern "C" int orbfe_essgraph_create(int device, int max_vertices, int max_edges, int max_env_blocks, int max_points,
                                     orbfe_essgraph** out) {
  if (!out) return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_essgraph_create: bad argument");
  *out = nullptr;
  if (max_vertices < 1 || max_vertices > ORBFE_ESSGRAPH_MAX_VERTICES || max_edges < 1 || max_edges > ORBFE_ESSGRAPH_MAX_EDGES ||
      max_env_blocks < 1 || max_env_blocks > ORBFE_ESSGRAPH_MAX_ENV_BLOCKS || max_points < 0 ||
      max_points > ORBFE_ESSGRAPH_MAX_POINTS)
    return orbfe_set_error(ORBFE_ERR_ARG,
                           "orbfe_essgraph_create: max_vertices in 1..8192, max_edges in 1..65536, max_env_blocks in "
                           "1..524288, max_points in 0..1048576");
  orbfe_essgraph* h = new orbfe_essgraph();
  memset(&h->w, 0, sizeof(h->w));
  h->max_v = max_vertices, h->max_e = max_edges, h->max_blk = max_env_blocks, h->max_p = max_points;
  if (device < 0) {
    *out = h;
    return ORBFE_OK;
  }
  const int open_st = orbfe_dev_open(h, device, "orbfe_essgraph_create");
  if (open_st != ORBFE_OK) {
    orbfe_essgraph_destroy(h);
    return open_st;
  }
  h->pool_bytes = eg_carve(h, nullptr);
  ORBFE_CREATE_HIP(h, orbfe_essgraph_destroy, hipMalloc(&h->d_pool, h->pool_bytes));
  ORBFE_CREATE_HIP(h, orbfe_essgraph_destroy, hipHostMalloc(&h->h_rec, sizeof(LmRec), hipHostMallocDefault));
  eg_carve(h, h->d_pool);
  *out = h;
  return ORBFE_OK;
}

extern "C" int orbfe_essgraph_destroy(orbfe_essgraph* h) {
  if (!h) return ORBFE_OK;
  if (orbfe_dev_close(h)) {
    hipFree(h->d_pool);
    if (h->h_rec) hipHostFree(h->h_rec);
  }
  delete h;
  return ORBFE_OK;
}

namespace {
inline unsigned eg_grid(size_t n) { return (unsigned)((n + EG_BLOCK - 1) / EG_BLOCK); }

// eg_run's backend over the handle's device workspace
struct EgDevBackend {
  orbfe_essgraph* h;
  EgWs w;

  template <class T>
  int up(const T* dst, const T* src, size_t count) {
    if (count == 0) return ORBFE_OK;
    ORBFE_HIP_CHECK(hipMemcpyAsync(const_cast<T*>(dst), src, sizeof(T) * count, hipMemcpyHostToDevice, h->stream));
    ORBFE_HIP_CHECK(hipStreamSynchronize(h->stream));  // the source may be pageable and short-lived
    return ORBFE_OK;
  }

  int start(const EgIn& in, const EgPlan& P) {
    w = h->w;
    w.nv = in.nv, w.ne = in.ne, w.ns = P.ns, w.nblk = (int)P.nblk, w.nob = P.nob, w.np = in.np;
    w.fix_scale = in.fix_scale, w.fixed = in.fixed;
    int st;
#define EG_UP(dst, src, count) \
  if ((st = up(dst, src, count)) != ORBFE_OK) return st
    EG_UP(w.tcw, in.tcw, 12 * (size_t)in.nv);
    EG_UP(w.corr_of_v, P.corr_of_v.data(), P.corr_of_v.size());
    EG_UP(w.nonc_of_v, P.nonc_of_v.data(), P.nonc_of_v.size());
    EG_UP(w.corr, in.corr, 8 * (size_t)in.ncorr);
    EG_UP(w.nonc, in.nonc, 8 * (size_t)in.nnonc);
    EG_UP(w.e_i, in.e_i, (size_t)in.ne);
    EG_UP(w.e_j, in.e_j, (size_t)in.ne);
    EG_UP(w.e_kind, in.e_kind, (size_t)in.ne);
    EG_UP(w.xw, in.xw, 3 * (size_t)in.np);
    EG_UP(w.p_ref, in.p_ref, (size_t)in.np);
    EG_UP(w.slot_of_v, P.slot_of_v.data(), P.slot_of_v.size());
    EG_UP(w.v_of_slot, P.v_of_slot.data(), P.v_of_slot.size());
    EG_UP(w.ve_begin, P.ve_begin.data(), P.ve_begin.size());
    EG_UP(w.ve_edge, P.ve_edge.data(), P.ve_edge.size());
    EG_UP(w.row_first, P.row_first.data(), P.row_first.size());
    EG_UP(w.row_off, P.row_off.data(), P.row_off.size());
    EG_UP(w.ob_begin, P.ob_begin.data(), P.ob_begin.size());
    EG_UP(w.ob_pos, P.ob_pos.data(), P.ob_pos.size());
    EG_UP(w.ob_edge, P.ob_edge.data(), P.ob_edge.size());
    EG_UP(w.col_begin, P.col_begin.data(), P.col_begin.size());
    EG_UP(w.col_row, P.col_row.data(), P.col_row.size());
#undef EG_UP
    if (w.ns > 0) ORBFE_HIP_CHECK(hipMemsetAsync(w.x, 0, sizeof(double) * 7 * (size_t)w.ns, h->stream));
    if (w.nv > 0) ORBFE_LAUNCH("k_eg_vertex_setup", k_eg_vertex_setup, dim3(eg_grid(w.nv)), dim3(EG_BLOCK), 0, h->stream, w);
    if (w.ne > 0) ORBFE_LAUNCH("k_eg_edge_setup", k_eg_edge_setup, dim3(eg_grid(w.ne)), dim3(EG_BLOCK), 0, h->stream, w);
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
    ORBFE_LAUNCH("k_eg_linearize", k_eg_linearize, dim3((w.ne + EG_LIN_EDGES - 1) / EG_LIN_EDGES),
                 dim3(EG_LIN_LANES * EG_LIN_EDGES), 0, h->stream, w);
    ORBFE_HIP_CHECK(hipMemsetAsync(w.H, 0, sizeof(double) * 49 * (size_t)w.nblk, h->stream));
    ORBFE_LAUNCH("k_eg_assemble", k_eg_assemble, dim3(w.ns + w.nob), dim3(EG_LANES), 0, h->stream, w);
    ORBFE_LAUNCH("k_eg_reduce", k_eg_reduce, dim3(1), dim3(EG_LANES), 0, h->stream, w, 0, 0.0);
    return read_rec(out);
  }

  int trial(double lambda, LmRec* out) {
    ORBFE_HIP_CHECK(hipMemsetAsync(w.rec, 0, sizeof(LmRec), h->stream));
    ORBFE_HIP_CHECK(hipMemcpyAsync(w.L, w.H, sizeof(double) * 49 * (size_t)w.nblk, hipMemcpyDeviceToDevice, h->stream));
    ORBFE_LAUNCH("k_eg_lambda", k_eg_lambda, dim3(eg_grid(7 * (size_t)w.ns)), dim3(EG_BLOCK), 0, h->stream, w, lambda);
    ORBFE_LAUNCH("k_eg_factor", k_eg_factor, dim3(1), dim3(EG_FACTOR_THREADS), 0, h->stream, w);
    ORBFE_LAUNCH("k_eg_update", k_eg_update, dim3(eg_grid(w.nv)), dim3(EG_BLOCK), 0, h->stream, w);
    ORBFE_LAUNCH("k_eg_chi", k_eg_chi, dim3(eg_grid(w.ne)), dim3(EG_BLOCK), 0, h->stream, w);
    ORBFE_LAUNCH("k_eg_reduce", k_eg_reduce, dim3(1), dim3(EG_LANES), 0, h->stream, w, 1, lambda);
    return read_rec(out);
  }

  int accept() {  // discardTop: the trial estimates become the accepted ones
    double* t = w.est;
    w.est = w.tri, w.tri = t;
    return ORBFE_OK;
  }

  int finish(float* tcw, float* xw) {
    ORBFE_LAUNCH("k_eg_finish", k_eg_finish, dim3(eg_grid((size_t)w.np + w.nv)), dim3(EG_BLOCK), 0, h->stream, w);
    ORBFE_HIP_CHECK(hipGetLastError());
    ORBFE_HIP_CHECK(hipMemcpyAsync(tcw, w.out_tcw, sizeof(float) * 12 * (size_t)w.nv, hipMemcpyDeviceToHost, h->stream));
    if (w.np > 0)
      ORBFE_HIP_CHECK(hipMemcpyAsync(xw, w.out_xw, sizeof(float) * 3 * (size_t)w.np, hipMemcpyDeviceToHost, h->stream));
    ORBFE_HIP_CHECK(hipStreamSynchronize(h->stream));
    return ORBFE_OK;
  }
};
}  // namespace

// the boundary: everything a kernel will use as an index
static int eg_check(const orbfe_essgraph* h, const orbfe_essgraph_problem_t* p, const orbfe_essgraph_result_t* r) {
  if (p->n_vertices < 1 || p->n_edges < 0 || p->n_points < 0 || p->n_corrected < 0 || p->n_noncorrected < 0)
    return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_essgraph_solve: a count below its minimum");
  if (p->n_vertices > ORBFE_ESSGRAPH_MAX_VERTICES || p->n_edges > ORBFE_ESSGRAPH_MAX_EDGES || p->n_points > ORBFE_ESSGRAPH_MAX_POINTS)
    return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_essgraph_solve: problem above the hard caps");
  if (p->n_vertices > h->max_v || p->n_edges > h->max_e || p->n_points > h->max_p)
    return orbfe_set_error(ORBFE_ERR_CAPACITY, "orbfe_essgraph_solve: problem above the handle's bounds");
  if (p->n_corrected > p->n_vertices || p->n_noncorrected > p->n_vertices)
    return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_essgraph_solve: more map entries than vertices");
  if (!p->tcw || !r->tcw || (p->n_corrected > 0 && (!p->corrected_idx || !p->corrected_sim3)) ||
      (p->n_noncorrected > 0 && (!p->noncorrected_idx || !p->noncorrected_sim3)) ||
      (p->n_edges > 0 && (!p->edge_i || !p->edge_j || !p->edge_kind)) || (p->n_points > 0 && (!p->xw || !p->point_ref || !r->xw)))
    return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_essgraph_solve: null array");
  const int nv = p->n_vertices;
  if (p->fixed_vertex < 0 || p->fixed_vertex >= nv) return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_essgraph_solve: fixed_vertex out of range");
  for (int m = 0; m < 2; m++) {
    const int n = m ? p->n_noncorrected : p->n_corrected;
    const int* idx = m ? p->noncorrected_idx : p->corrected_idx;
    std::vector<uint8_t> seen(nv, 0);
    for (int k = 0; k < n; k++) {
      if (idx[k] < 0 || idx[k] >= nv) return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_essgraph_solve: a map's vertex index out of range");
      if (seen[idx[k]]) return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_essgraph_solve: a keyframe listed twice in a map");
      seen[idx[k]] = 1;
    }
  }
  for (int e = 0; e < p->n_edges; e++) {
    if (p->edge_i[e] < 0 || p->edge_i[e] >= nv || p->edge_j[e] < 0 || p->edge_j[e] >= nv)
      return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_essgraph_solve: edge vertex index out of range");
    if (p->edge_i[e] == p->edge_j[e]) return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_essgraph_solve: an edge with i == j");
    if (p->edge_kind[e] > 1) return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_essgraph_solve: edge kind above 1");
  }
  for (int q = 0; q < p->n_points; q++)
    if (p->point_ref[q] < 0 || p->point_ref[q] >= nv) return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_essgraph_solve: point_ref out of range");
  return ORBFE_OK;
}

extern "C" int orbfe_essgraph_solve(orbfe_essgraph* h, const orbfe_essgraph_problem_t* p, orbfe_essgraph_result_t* r) {
  if (!h || !p || !r) return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_essgraph_solve: bad argument");
  int st = eg_check(h, p, r);
  if (st != ORBFE_OK) return st;
  EgIn in = {p->n_vertices, p->fixed_vertex, p->fix_scale ? 1 : 0, p->tcw, p->n_corrected, p->corrected_idx, p->corrected_sim3,
             p->n_noncorrected, p->noncorrected_idx, p->noncorrected_sim3, p->n_edges, p->edge_i, p->edge_j, p->edge_kind,
             p->n_points, p->xw, p->point_ref};
  EgPlan plan;
  eg_plan_envelope(in, &plan);
  if (plan.nblk > h->max_blk) return orbfe_set_error(ORBFE_ERR_CAPACITY, "orbfe_essgraph_solve: envelope above max_env_blocks");
  if (h->device < 0) return orbfe_set_error(ORBFE_ERR_STATE, "essential graph optimizer is host-only (device < 0)");
  eg_plan_rest(in, &plan);
  EgOut o;
  ORBFE_HIP_CHECK(hipSetDevice(h->device));
  EgDevBackend b = {h, h->w};
  st = eg_run(b, in, plan, &o);
  if (st != ORBFE_OK) return st;
  memcpy(r->tcw, o.tcw.data(), sizeof(float) * o.tcw.size());
  if (p->n_points > 0) memcpy(r->xw, o.xw.data(), sizeof(float) * o.xw.size());
  memcpy(&r->trace, &o.trace, sizeof(r->trace));
  return ORBFE_OK;
}
