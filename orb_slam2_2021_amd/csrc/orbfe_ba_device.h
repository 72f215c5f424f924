// orbfe_ba_device.h -- what the two bundle adjusters share on the device side (orbfe_lba.hip: local,
// dense Schur; orbfe_gba.hip: global, envelope Schur): the stage kernels over orbfe_lba_core.h, the
// wavefront tree, the carve of the LbaWs part of a handle's pool, the backend half that uploads a plan,
// launches the stages and reads the record back, and the CSR part of the boundary check. Each solver adds
// its own reduced system between begin_trial and end_trial. Included by those two files only; the kernels
// are templates or static, so each translation unit holds its own.
//   k_ba_edge    per active edge: error, robust weight and (linearisation) Jacobians and the edge's own
//                Hll, bl, Hpl, Hpp, bp products
//   k_ba_point   per point: Hll, bl, chi2 share over its edges in order
//   k_ba_pose    one wavefront per slot: Hpp(i,i), bp_i by the 64-lane rule
//   k_ba_dinv    per point: Dinv = (Hll + lambda I)^-1, db
//   k_ba_update  per point: back-substitution and the trial point; per keyframe: exp(x) * T
//   k_ba_reduce  one wavefront: the total chi2 with computeLambdaInit's maximum or computeScale
// The kernel timer sees them under each solver's own labels (BaNames): k_lba_edge, k_gba_edge, ...
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdio>
#include <vector>

#include "orbfe_device.h"
#include "orbfe_ktimer.h"
#include "orbfe_lba_core.h"
#include "orbfe_stage.h"

#define BA_BLOCK 128

template <bool FULL>
__global__ __launch_bounds__(BA_BLOCK) void k_ba_edge(LbaWs w, int trial) {
  const int e = blockIdx.x * BA_BLOCK + threadIdx.x;
  if (e < w.ne) lba_edge<FULL>(w, e, trial != 0);
}

template <bool FULL>
__global__ __launch_bounds__(BA_BLOCK) void k_ba_point(LbaWs w) {
  const int p = blockIdx.x * BA_BLOCK + threadIdx.x;
  if (p < w.np) lba_point_sum<FULL>(w, p);
}

// the tree: lane 0 ends with s[0] of the host's s[l] += s[l + stride]
__device__ inline double ba_tree(double v) {
#pragma unroll
  for (int stride = LBA_LANES / 2; stride >= 1; stride >>= 1) v = v + __shfl_down(v, stride);
  return v;
}

static __global__ __launch_bounds__(LBA_LANES) void k_ba_pose(LbaWs w) {
  const int f = w.free_of_slot[blockIdx.x];
  double acc[27];
  lba_pose_lane(w, f, threadIdx.x, acc);
#pragma unroll
  for (int k = 0; k < 27; k++) acc[k] = ba_tree(acc[k]);
  if (threadIdx.x == 0) lba_pose_finish(w, f, acc);
}

static __global__ __launch_bounds__(BA_BLOCK) void k_ba_dinv(LbaWs w, double lambda) {
  const int p = blockIdx.x * BA_BLOCK + threadIdx.x;
  if (p < w.np) lba_point_dinv(w, p, lambda);
}

static __global__ __launch_bounds__(BA_BLOCK) void k_ba_update(LbaWs w) {
  const int i = blockIdx.x * BA_BLOCK + threadIdx.x;
  if (i < w.np) {
    if (!w.rec->fail) lba_point_backsub(w, i);  // after a failed solve x keeps its last values
    lba_update_point(w, i);
  } else if (i - w.np < w.nk) {
    lba_update_kf(w, i - w.np);
  }
}

static __global__ __launch_bounds__(LBA_LANES) void k_ba_reduce(LbaWs w, int mode, double lambda) {
  double part[2];
  lba_reduce_lane(w, threadIdx.x, mode, lambda, part);
  const double chi = ba_tree(part[0]);
  double other;
  if (mode) {
    other = ba_tree(part[1]);
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

// The LbaWs part of a handle's device pool (a counting block only sizes it). nf: the bound on the free keyframes, which is the bound on the slots;
// dense: the local adjuster's S, Lm, Mm (the global one's reduced system is its envelope)
inline void ba_carve(OrbfeStage& pool, LbaWs& w, size_t nk, size_t nf, size_t np, size_t ne, bool dense) {
  const size_t n = 6 * nf;
  pool.take(w.cam, 5 * nk);
  pool.take(w.kf_free, nk);
  pool.take(w.edge_begin, np + 1);
  pool.take(w.e_kf, ne);
  pool.take(w.e_pt, ne);
  pool.take(w.e_obs, 3 * ne);
  pool.take(w.e_w, ne);
  pool.take(w.e_stereo, ne);
  pool.take(w.kl_begin, nf * LBA_LANES + 1);
  pool.take(w.kl_edge, ne);
  pool.take(w.e_active, ne);
  pool.take(w.p_active, np);
  pool.take(w.slot_of_free, nf);
  pool.take(w.free_of_slot, nf);
  pool.take(w.est_T, 7 * nk);
  pool.take(w.tri_T, 7 * nk);
  pool.take(w.est_X, 3 * np);
  pool.take(w.tri_X, 3 * np);
  pool.take(w.e_err, 3 * ne);
  pool.take(w.e_prod, LBA_EDGE_DOUBLES * ne);
  pool.take(w.p_hll, 9 * np);
  pool.take(w.p_bl, 3 * np);
  pool.take(w.p_chi, np);
  pool.take(w.p_dinv, 9 * np);
  pool.take(w.p_db, 3 * np);
  pool.take(w.p_xl, 3 * np);
  pool.take(w.hpp, 21 * nf);
  pool.take(w.bp, 6 * nf);
  if (dense) pool.take(w.S, n * n);
  pool.take(w.bs, n);
  if (dense) pool.take(w.Lm, n * n), pool.take(w.Mm, n * n);
  pool.take(w.d, n);
  pool.take(w.y, n);
  pool.take(w.xp, n);
  pool.take(w.rec, 1);
}

inline unsigned ba_grid(long long n, int block = BA_BLOCK) { return (unsigned)((n + block - 1) / block); }

// the kernel timer's labels of one solver's stages
struct BaNames {
  const char *edge, *point, *pose, *dinv, *update, *edge_trial, *point_chi, *reduce;
};

// in a backend's method: upload or return the status
#define BA_UP(dst, src, count) \
  if ((st = up(dst, src, count)) != ORBFE_OK) return st

// lba_round's backend over a handle's device workspace, up to the reduced system: a solver's trial is
// begin_trial, its own Schur complement and solve, end_trial
struct BaDevBackend {
  hipStream_t stream;
  LmRec* h_rec;  // pinned
  LbaWs w;
  const BaNames* nm;

  template <class T>
  int up(const T* dst, const T* src, size_t count) {
    if (count == 0) return ORBFE_OK;
    ORBFE_HIP_CHECK(hipMemcpyAsync(const_cast<T*>(dst), src, sizeof(T) * count, hipMemcpyHostToDevice, stream));
    ORBFE_HIP_CHECK(hipStreamSynchronize(stream));  // the source may be pageable and short-lived
    return ORBFE_OK;
  }

  // the counts and the plan; the caller has set w to the handle's pointers and sets its own deltas
  int start(const LbaPlan& P) {
    w.nk = P.nk, w.nfree = P.nfree, w.np = P.np, w.ne = P.ne, w.nslot = 0, w.kernel_on = 1;
    int st;
    BA_UP(w.cam, P.cam.data(), P.cam.size());
    BA_UP(w.kf_free, P.kf_free.data(), P.kf_free.size());
    BA_UP(w.edge_begin, P.edge_begin, (size_t)P.np + 1);
    BA_UP(w.e_kf, P.e_kf, (size_t)P.ne);
    BA_UP(w.e_pt, P.e_pt.data(), P.e_pt.size());
    BA_UP(w.e_obs, P.e_obs.data(), P.e_obs.size());
    BA_UP(w.e_w, P.e_w.data(), P.e_w.size());
    BA_UP(w.e_stereo, P.e_stereo.data(), P.e_stereo.size());
    BA_UP(w.kl_begin, P.kl_begin.data(), P.kl_begin.size());
    BA_UP(w.kl_edge, P.kl_edge.data(), P.kl_edge.size());
    BA_UP((const double*)w.est_T, P.T0.data(), P.T0.size());
    BA_UP((const double*)w.tri_T, P.T0.data(), P.T0.size());
    BA_UP((const double*)w.est_X, P.X0.data(), P.X0.size());
    BA_UP((const double*)w.tri_X, P.X0.data(), P.X0.size());
    ORBFE_HIP_CHECK(hipMemsetAsync(w.e_err, 0, sizeof(double) * 3 * (size_t)w.ne, stream));
    return ORBFE_OK;
  }

  // n_xp: the doubles of xp the solver clears before a round's first solve
  int begin_round(const LbaActive& A, bool kernel_on, size_t n_xp) {
    int st;
    BA_UP(w.e_active, A.e_active.data(), A.e_active.size());
    BA_UP(w.p_active, A.p_active.data(), A.p_active.size());
    BA_UP(w.slot_of_free, A.slot_of_free.data(), A.slot_of_free.size());
    BA_UP(w.free_of_slot, A.free_of_slot.data(), A.free_of_slot.size());
    w.nslot = A.nslot, w.kernel_on = kernel_on ? 1 : 0;
    if (n_xp > 0) ORBFE_HIP_CHECK(hipMemsetAsync(w.xp, 0, sizeof(double) * n_xp, stream));
    ORBFE_HIP_CHECK(hipMemsetAsync(w.p_xl, 0, sizeof(double) * 3 * (size_t)w.np, stream));
    return ORBFE_OK;
  }

  int read_rec(LmRec* out) {
    ORBFE_HIP_CHECK(hipGetLastError());
    ORBFE_HIP_CHECK(hipMemcpyAsync(h_rec, w.rec, sizeof(LmRec), hipMemcpyDeviceToHost, stream));
    ORBFE_HIP_CHECK(hipStreamSynchronize(stream));
    *out = *h_rec;
    return ORBFE_OK;
  }

  int linearize(LmRec* out) {
    ORBFE_HIP_CHECK(hipMemsetAsync(w.rec, 0, sizeof(LmRec), stream));
    ORBFE_LAUNCH(nm->edge, k_ba_edge<true>, dim3(ba_grid(w.ne)), dim3(BA_BLOCK), 0, stream, w, 0);
    ORBFE_LAUNCH(nm->point, k_ba_point<true>, dim3(ba_grid(w.np)), dim3(BA_BLOCK), 0, stream, w);
    if (w.nslot > 0) ORBFE_LAUNCH(nm->pose, k_ba_pose, dim3(w.nslot), dim3(LBA_LANES), 0, stream, w);
    ORBFE_LAUNCH(nm->reduce, k_ba_reduce, dim3(1), dim3(LBA_LANES), 0, stream, w, 0, 0.0);
    return read_rec(out);
  }

  int begin_trial(double lambda) {
    ORBFE_HIP_CHECK(hipMemsetAsync(w.rec, 0, sizeof(LmRec), stream));
    ORBFE_LAUNCH(nm->dinv, k_ba_dinv, dim3(ba_grid(w.np)), dim3(BA_BLOCK), 0, stream, w, lambda);
    return ORBFE_OK;
  }

  int end_trial(double lambda, LmRec* out) {
    ORBFE_LAUNCH(nm->update, k_ba_update, dim3(ba_grid((long long)w.np + w.nk)), dim3(BA_BLOCK), 0, stream, w);
    ORBFE_LAUNCH(nm->edge_trial, k_ba_edge<false>, dim3(ba_grid(w.ne)), dim3(BA_BLOCK), 0, stream, w, 1);
    ORBFE_LAUNCH(nm->point_chi, k_ba_point<false>, dim3(ba_grid(w.np)), dim3(BA_BLOCK), 0, stream, w);
    ORBFE_LAUNCH(nm->reduce, k_ba_reduce, dim3(1), dim3(LBA_LANES), 0, stream, w, 1, lambda);
    return read_rec(out);
  }

  int accept() {  // discardTop: the trial estimates become the accepted ones
    double* t = w.est_T;
    w.est_T = w.tri_T, w.tri_T = t;
    t = w.est_X;
    w.est_X = w.tri_X, w.tri_X = t;
    return ORBFE_OK;
  }

  int finish(double* T, double* X) {
    ORBFE_HIP_CHECK(hipMemcpyAsync(T, w.est_T, sizeof(double) * 7 * (size_t)w.nk, hipMemcpyDeviceToHost, stream));
    ORBFE_HIP_CHECK(hipMemcpyAsync(X, w.est_X, sizeof(double) * 3 * (size_t)w.np, hipMemcpyDeviceToHost, stream));
    ORBFE_HIP_CHECK(hipStreamSynchronize(stream));
    return ORBFE_OK;
  }
};

// The boundary's walk over the points' edge lists: edge_begin a CSR over n_edges, every keyframe index in
// range, no keyframe twice under one point. who: the entry point, for the message.
inline int ba_check_csr(const char* who, int n_kf, int n_points, int n_edges, const int* edge_begin, const int* edge_kf) {
  char msg[160];
  auto err = [&](const char* what) {
    snprintf(msg, sizeof(msg), "%s: %s", who, what);
    return orbfe_set_error(ORBFE_ERR_ARG, msg);
  };
  if (edge_begin[0] != 0 || edge_begin[n_points] != n_edges) return err("edge_begin is not a CSR over n_edges");
  std::vector<int> seen(n_kf > 0 ? n_kf : 1, -1);
  for (int q = 0; q < n_points; q++) {
    const int b = edge_begin[q], e = edge_begin[q + 1];
    if (b > e || b < 0 || e > n_edges) return err("edge_begin is not a CSR over n_edges");
    for (int i = b; i < e; i++) {
      const int kf = edge_kf[i];
      if (kf < 0 || kf >= n_kf) return err("keyframe index out of range");
      if (seen[kf] == q) return err("a keyframe listed twice under one point");
      seen[kf] = q;
    }
  }
  return ORBFE_OK;
}
