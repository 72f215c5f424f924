// orbfe_triangulate.hip -- LocalMapping::CreateNewMapPoints' geometry on the GPU
// (include/orbfe_triangulate.h): SearchForTriangulation's matches in, map points out.
//
//   k_tri_zero     one thread per pair: nnew = 0
//   k_triangulate  grid (ceil(max n1 / 256), n_pairs), 256 threads: a block compacts the matched
//                  keypoints of its 256 (one ballot per wavefront, a four-entry prefix in LDS), then
//                  its first k threads take one match each (orbfe_triangulate_core.h)
//
// Bounds by construction: a thread reads match12 / writes status only at i < n1 <= kf1.n (the host
// checked kf1.n against the caller's buffers' contract); a compacted entry carries 0 <= idx2 < kf2.n
// (tested before it is listed) and both octaves are tested against nlevels before a level table is
// read; the LDS list has one slot per thread of the block and k <= 256.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/orbfe_triangulate.h"
#include "orbfe_device.h"
#include "orbfe_ktimer.h"
#include "orbfe_match_internal.h"
#include "orbfe_triangulate_core.h"

#define TRI_THREADS 256
#define TRI_WAVES (TRI_THREADS / 64)

__global__ __launch_bounds__(64) void k_tri_zero(const orbfe_tri_pair* pairs, int n_pairs) {
  const int p = blockIdx.x * 64 + threadIdx.x;
  if (p < n_pairs) *pairs[p].nnew = 0;
}

__device__ __forceinline__ TriCam tri_cam(const orbfe_frame_view& f) {
  TriCam c;
  c.fx = f.fx;
  c.fy = f.fy;
  c.cx = f.cx;
  c.cy = f.cy;
  c.invfx = 1.0f / f.fx;  // invfx = 1.0f / fx (Frame.cc, KeyFrame.cc)
  c.invfy = 1.0f / f.fy;
  c.bf = f.bf;
  c.b = f.b;
  return c;
}

// The keypoint's observation; false when its octave is outside the KeyFrame's level tables.
__device__ __forceinline__ bool tri_obs(const orbfe_frame_view& f, const orbfe_tri_keyframe& t, int idx, TriObs& o) {
  const orbfe_keypoint kp = f.keys_un[idx];
  o.x = kp.x;
  o.y = kp.y;
  o.ur = f.u_right[idx];
  o.depth = t.depth[idx];
  o.kx = t.keys_xy ? t.keys_xy[2 * (size_t)idx] : kp.x;
  o.ky = t.keys_xy ? t.keys_xy[2 * (size_t)idx + 1] : kp.y;
  const bool ok = kp.octave >= 0 && kp.octave < f.nlevels;
  o.sigma2 = ok ? f.level_sigma2[kp.octave] : 0.0f;
  o.scale = ok ? f.scale_factors[kp.octave] : 0.0f;
  return ok;
}

__global__ __launch_bounds__(TRI_THREADS) void k_triangulate(const orbfe_tri_pair* pairs) {
  __shared__ int s_wcnt[TRI_WAVES];
  __shared__ int s_i1[TRI_THREADS], s_i2[TRI_THREADS];
  const orbfe_tri_pair& P = pairs[blockIdx.y];
  int n1 = P.kf1.n;
  if (P.kf1_n_dev) n1 = min(max(*P.kf1_n_dev, 0), n1);
  const int base = blockIdx.x * TRI_THREADS;
  if (base >= n1) return;  // block-uniform
  const int t = threadIdx.x, lane = lane_id(), w = wave_id();
  const int i = base + t;
  int m = -1;
  if (i < n1) {
    m = P.match12[i];
    if (m >= P.kf2.n) {
      P.status[i] = ORBFE_TRI_REJ_BAD_MATCH;
      m = -1;
    } else if (m < 0) {
      P.status[i] = ORBFE_TRI_NO_MATCH;
    }
  }
  // compaction: about one keypoint in ten has a match, so the matches of the block's four
  // wavefronts are packed into its first wavefront(s) before the SVD
  const uint64_t has = wave_ballot(m >= 0);
  if (lane == 0) s_wcnt[w] = __popcll(has);
  __syncthreads();
  int off = 0, k = 0;
#pragma unroll
  for (int q = 0; q < TRI_WAVES; q++) {
    const int c = s_wcnt[q];
    off += q < w ? c : 0;
    k += c;
  }
  if (m >= 0) {
    const int slot = off + prefix_in_wave(has);  // < k <= TRI_THREADS
    s_i1[slot] = i;
    s_i2[slot] = m;
  }
  __syncthreads();
  if (w * 64 >= k) return;  // wave-uniform: nothing left for this wavefront
  bool accepted = false;
  if (t < k) {
    const int idx1 = s_i1[t], idx2 = s_i2[t];
    TriObs o1, o2;
    const bool ok1 = tri_obs(P.kf1, P.t1, idx1, o1);
    const bool ok2 = tri_obs(P.kf2, P.t2, idx2, o2);
    int st = ORBFE_TRI_REJ_BAD_OCTAVE;
    float X[3] = {0.0f, 0.0f, 0.0f};
    if (ok1 && ok2) {
      const float ratio_factor = P.kf1.nlevels > 1 ? 1.5f * P.kf1.scale_factors[1] : 1.5f;
      st = tri_match(P.t1.tcw, P.t1.ow, tri_cam(P.kf1), o1, P.t2.tcw, P.t2.ow, tri_cam(P.kf2), o2, ratio_factor, X);
    }
    P.status[idx1] = (int8_t)st;
    if (st > 0) {
      accepted = true;
      P.x3d[3 * (size_t)idx1] = X[0];
      P.x3d[3 * (size_t)idx1 + 1] = X[1];
      P.x3d[3 * (size_t)idx1 + 2] = X[2];
      // AddMapPoint (:445-446): the keypoints now hold a MapPoint with observations
      if (P.mark1) P.mark1[idx1] = ORBFE_MP_OBSERVED;
      if (P.mark2) P.mark2[idx2] = ORBFE_MP_OBSERVED;
    }
  }
  const uint64_t acc = wave_ballot(accepted);
  if (lane == 0 && acc) atomicAdd(P.nnew, (int)__popcll(acc));
}

// ------------------------------------------------------------------------------------------
// host

static bool tri_kf_ok(const orbfe_frame_view& f, const orbfe_tri_keyframe& t, int max_n) {
  if (f.n < 0 || f.n > max_n) return false;
  if (f.n > 0 && (!f.keys_un || !f.u_right || !f.scale_factors || !f.level_sigma2 || !t.depth)) return false;
  return true;
}

// Host checks of one pair, before any launch. `what` prefixes the message.
static int tri_check_pair(const char* what, const orbfe_tri_pair& p) {
  static thread_local char msg[160];
  auto fail = [&](int code, const char* why) {
    snprintf(msg, sizeof(msg), "%s: %s", what, why);
    return orbfe_set_error(code, msg);
  };
  if (p.kf1.n > ORBFE_TRI_MAX_KEYS) return fail(ORBFE_ERR_CAPACITY, "KF1 has more than 8192 keypoints");
  if (p.kf2.n > ORBFE_TRI_MAX_KF2_KEYS) return fail(ORBFE_ERR_CAPACITY, "KF2 has more than 16384 keypoints");
  if (p.kf1.nlevels < 1 || p.kf1.nlevels > ORBFE_TRI_MAX_LEVELS || p.kf2.nlevels < 1 ||
      p.kf2.nlevels > ORBFE_TRI_MAX_LEVELS)
    return fail(ORBFE_ERR_ARG, "nlevels outside 1..32");
  if (!tri_kf_ok(p.kf1, p.t1, ORBFE_TRI_MAX_KEYS) || !tri_kf_ok(p.kf2, p.t2, ORBFE_TRI_MAX_KF2_KEYS))
    return fail(ORBFE_ERR_ARG, "negative n or a NULL KeyFrame array (keys_un, u_right, scale_factors, level_sigma2, depth)");
  if (!p.nnew || (p.kf1.n > 0 && (!p.match12 || !p.status || !p.x3d)))
    return fail(ORBFE_ERR_ARG, "NULL match12, status, x3d or nnew");
  return ORBFE_OK;
}

// Room for `bytes` of pair records in device memory and in the host bytes they upload from.
static int tri_reserve(orbfe_matcher* m, size_t bytes) {
  if (bytes > m->d_tri_bytes) {
    hipFree(m->d_tri);
    m->d_tri = nullptr;
    m->d_tri_bytes = 0;
    ORBFE_HIP_CHECK(hipMalloc(&m->d_tri, bytes));
    m->d_tri_bytes = bytes;
  }
  m->tri_host.resize(bytes);
  return ORBFE_OK;
}

static void tri_launch(hipStream_t s, const orbfe_tri_pair* d_pairs, int n_pairs, int max_n1) {
  ORBFE_LAUNCH("k_triangulate", k_triangulate, dim3(std::max(1, (max_n1 + TRI_THREADS - 1) / TRI_THREADS), n_pairs),
               dim3(TRI_THREADS), 0, s, d_pairs);
}

extern "C" int orbfe_triangulate_batch_device(orbfe_matcher* m, int n_pairs, const orbfe_tri_pair* pairs,
                                              void* stream) {
  if (n_pairs < 0 || n_pairs > ORBFE_TRI_MAX_PAIRS)
    return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_triangulate_batch_device: n_pairs outside 0..4096");
  if (n_pairs > 0 && !pairs) return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_triangulate_batch_device: pairs is NULL");
  int max_n1 = 0;
  for (int p = 0; p < n_pairs; p++) {
    const int st = tri_check_pair("orbfe_triangulate_batch_device", pairs[p]);
    if (st) return st;
    max_n1 = std::max(max_n1, pairs[p].kf1.n);
  }
  if (!m) return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_triangulate_batch_device: matcher is NULL");
  if (n_pairs == 0) return ORBFE_OK;
  ORBFE_HIP_CHECK(hipSetDevice(m->device));
  hipStream_t s = stream ? (hipStream_t)stream : m->stream;
  const size_t bytes = sizeof(orbfe_tri_pair) * (size_t)n_pairs;
  const int st = tri_reserve(m, bytes);
  if (st) return st;
  std::memcpy(m->tri_host.data(), pairs, bytes);
  ORBFE_HIP_CHECK(hipMemcpyAsync(m->d_tri, m->tri_host.data(), bytes, hipMemcpyHostToDevice, s));
  const orbfe_tri_pair* d = reinterpret_cast<const orbfe_tri_pair*>(m->d_tri);
  ORBFE_LAUNCH("k_tri_zero", k_tri_zero, dim3((n_pairs + 63) / 64), dim3(64), 0, s, d, n_pairs);
  tri_launch(s, d, n_pairs, max_n1);
  ORBFE_HIP_CHECK(hipGetLastError());
  return ORBFE_OK;
}

extern "C" int orbfe_triangulate_matches(orbfe_matcher* m, const orbfe_frame_view* kf1,
                                         const orbfe_tri_keyframe* t1, const orbfe_frame_view* kf2,
                                         const orbfe_tri_keyframe* t2, const int32_t* match12, int8_t* status,
                                         float* x3d, int* nnew) {
  if (!kf1 || !t1 || !kf2 || !t2) return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_triangulate_matches: NULL KeyFrame");
  orbfe_tri_pair P;
  std::memset(&P, 0, sizeof(P));
  P.kf1 = *kf1;
  P.kf2 = *kf2;
  P.t1 = *t1;
  P.t2 = *t2;
  P.match12 = match12;
  P.status = status;
  P.x3d = x3d;
  int32_t nn = 0;
  P.nnew = nnew ? &nn : nullptr;
  int st = tri_check_pair("orbfe_triangulate_matches", P);
  if (st) return st;
  if (!m) return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_triangulate_matches: matcher is NULL");
  ORBFE_HIP_CHECK(hipSetDevice(m->device));
  using namespace orbfe_mi;
  Arena ar;
  struct KfOff {
    size_t keys, ur, depth, xy, scale, sigma2;
  };
  auto plan = [&](const orbfe_frame_view& f) {
    const size_t n = (size_t)std::max(f.n, 1), l = (size_t)f.nlevels;
    KfOff o;
    o.keys = ar.add(sizeof(orbfe_keypoint) * n);
    o.ur = ar.add(4 * n);
    o.depth = ar.add(4 * n);
    o.xy = ar.add(8 * n);
    o.scale = ar.add(4 * l);
    o.sigma2 = ar.add(4 * l);
    return o;
  };
  const KfOff o1 = plan(*kf1), o2 = plan(*kf2);
  const size_t n1 = (size_t)std::max(kf1->n, 1);
  const size_t om = ar.add(4 * n1), ox = ar.add(12 * n1), os = ar.add(n1), on = ar.add(4);
  if ((st = ensure_arena(m, ar.total))) return st;
  uint8_t* A = m->arena;
  auto stage = [&](const KfOff& o, orbfe_frame_view& f, orbfe_tri_keyframe& t) {
    const size_t n = (size_t)f.n, l = (size_t)f.nlevels;
    if (n > 0) {
      stage_h2d(m, A + o.keys, f.keys_un, sizeof(orbfe_keypoint) * n);
      stage_h2d(m, A + o.ur, f.u_right, 4 * n);
      stage_h2d(m, A + o.depth, t.depth, 4 * n);
      if (t.keys_xy) stage_h2d(m, A + o.xy, t.keys_xy, 8 * n);
      stage_h2d(m, A + o.scale, f.scale_factors, 4 * l);
      stage_h2d(m, A + o.sigma2, f.level_sigma2, 4 * l);
    }
    f.keys_un = (const orbfe_keypoint*)(A + o.keys);
    f.u_right = (const float*)(A + o.ur);
    f.descriptors = nullptr;
    f.mp_state = nullptr;
    f.scale_factors = (const float*)(A + o.scale);
    f.level_sigma2 = (const float*)(A + o.sigma2);
    t.depth = (const float*)(A + o.depth);
    t.keys_xy = t.keys_xy ? (const float*)(A + o.xy) : nullptr;
  };
  stage(o1, P.kf1, P.t1);
  stage(o2, P.kf2, P.t2);
  if (kf1->n > 0) {
    stage_h2d(m, A + om, match12, 4 * (size_t)kf1->n);
    stage_h2d(m, A + ox, x3d, 12 * (size_t)kf1->n);  // entries without a point come back as they were
  }
  P.match12 = (const int32_t*)(A + om);
  P.x3d = (float*)(A + ox);
  P.status = (int8_t*)(A + os);
  P.nnew = (int32_t*)(A + on);
  if ((st = flush_h2d(m))) return st;
  if ((st = orbfe_triangulate_batch_device(m, 1, &P, m->stream))) return st;
  if (kf1->n > 0) {
    stage_d2h(m, status, P.status, (size_t)kf1->n);
    stage_d2h(m, x3d, P.x3d, 12 * (size_t)kf1->n);
  }
  stage_d2h(m, &nn, P.nnew, 4);
  if ((st = fetch_d2h(m))) return st;
  *nnew = nn;
  return ORBFE_OK;
}

extern "C" int orbfe_create_new_mappoints_device(orbfe_matcher* m, const orbfe_frame_view* kf1,
                                                 const orbfe_tri_keyframe* t1, const orbfe_feature_vector* fv1,
                                                 int n_nb, const orbfe_tri_neighbour* nbs, int32_t* match12,
                                                 int8_t* status, float* x3d, int32_t* nmatches, int32_t* nnew,
                                                 void* stream) {
  const char* fn = "orbfe_create_new_mappoints_device";
  static thread_local char msg[160];
  auto fail = [&](int code, const char* why) {
    snprintf(msg, sizeof(msg), "%s: %s", fn, why);
    return orbfe_set_error(code, msg);
  };
  if (n_nb < 0 || n_nb > ORBFE_TRI_MAX_NEIGHBOURS) return fail(ORBFE_ERR_ARG, "n_nb outside 0..64");
  if (!kf1 || !t1 || !fv1 || (n_nb > 0 && (!nbs || !nmatches || !nnew))) return fail(ORBFE_ERR_ARG, "NULL argument");
  auto search_ok = [](const orbfe_frame_view& f, const orbfe_feature_vector& fv) {
    return fv.n_nodes >= 0 && (fv.n_nodes == 0 || (fv.node_ids && fv.offsets && fv.indices)) &&
           (f.n == 0 || (f.descriptors && f.mp_state));
  };
  if (!search_ok(*kf1, *fv1)) return fail(ORBFE_ERR_ARG, "KF1 lacks descriptors, mp_state or its FeatureVector");
  std::vector<orbfe_tri_pair> tri((size_t)n_nb);
  std::vector<orbfe_sft_pair> sft((size_t)n_nb);
  for (int j = 0; j < n_nb; j++) {
    const orbfe_tri_neighbour& nb = nbs[j];
    orbfe_tri_pair& T = tri[j];
    std::memset(&T, 0, sizeof(T));
    T.kf1 = *kf1;
    T.kf2 = nb.kf;
    T.t1 = *t1;
    T.t2 = nb.t;
    T.match12 = match12 ? match12 + (size_t)j * kf1->n : nullptr;
    T.status = status ? status + (size_t)j * kf1->n : nullptr;
    T.x3d = x3d ? x3d + 3 * (size_t)j * kf1->n : nullptr;
    T.nnew = nnew + j;
    T.mark1 = const_cast<uint8_t*>(kf1->mp_state);
    T.mark2 = const_cast<uint8_t*>(nb.kf.mp_state);
    const int st = tri_check_pair(fn, T);
    if (st) return st;
    if (!search_ok(nb.kf, nb.fv)) return fail(ORBFE_ERR_ARG, "a neighbour lacks descriptors, mp_state or its FeatureVector");
    // a KeyFrame is its keypoints and its MapPoint slots: the same arrays twice are one KeyFrame
    if (nb.kf.n > 0 && kf1->n > 0 && (nb.kf.mp_state == kf1->mp_state || nb.kf.keys_un == kf1->keys_un))
      return fail(ORBFE_ERR_ARG, "a neighbour equals KF1");
    for (int q = 0; q < j; q++)
      if (nb.kf.n > 0 && nbs[q].kf.n > 0 &&
          (nb.kf.mp_state == nbs[q].kf.mp_state || nb.kf.keys_un == nbs[q].kf.keys_un))
        return fail(ORBFE_ERR_ARG, "a neighbour appears twice");
    orbfe_sft_pair& S = sft[j];
    std::memset(&S, 0, sizeof(S));
    S.kf1 = *kf1;
    S.kf2 = nb.kf;
    S.fv1 = *fv1;
    S.fv2 = nb.fv;
    std::memcpy(S.f12, nb.f12, sizeof(S.f12));
    S.ex = nb.ex;
    S.ey = nb.ey;
    S.match12 = const_cast<int32_t*>(T.match12);
    S.nmatches = nmatches + j;
  }
  if (!m) return fail(ORBFE_ERR_ARG, "matcher is NULL");
  if (n_nb == 0) return ORBFE_OK;
  ORBFE_HIP_CHECK(hipSetDevice(m->device));
  hipStream_t s = stream ? (hipStream_t)stream : m->stream;
  // one upload of every neighbour's two records, then three launches per neighbour
  const size_t tri_bytes = orbfe_al256(sizeof(orbfe_tri_pair) * (size_t)n_nb);
  const size_t bytes = tri_bytes + sizeof(orbfe_sft_pair) * (size_t)n_nb;
  const int st = tri_reserve(m, bytes);
  if (st) return st;
  std::memcpy(m->tri_host.data(), tri.data(), sizeof(orbfe_tri_pair) * (size_t)n_nb);
  std::memcpy(m->tri_host.data() + tri_bytes, sft.data(), sizeof(orbfe_sft_pair) * (size_t)n_nb);
  ORBFE_HIP_CHECK(hipMemcpyAsync(m->d_tri, m->tri_host.data(), bytes, hipMemcpyHostToDevice, s));
  const orbfe_tri_pair* d_tri = reinterpret_cast<const orbfe_tri_pair*>(m->d_tri);
  const orbfe_sft_pair* d_sft = reinterpret_cast<const orbfe_sft_pair*>(m->d_tri + tri_bytes);
  ORBFE_LAUNCH("k_tri_zero", k_tri_zero, dim3((n_nb + 63) / 64), dim3(64), 0, s, d_tri, n_nb);
  for (int j = 0; j < n_nb; j++) {
    // bOnlyStereo = false (:272); the matcher's own checkOri, as the caller constructed it (:219)
    orbfe_mi::sft_launch(s, d_sft + j, 1, std::max(1, fv1->n_nodes), 0, m->check_ori);
    tri_launch(s, d_tri + j, 1, kf1->n);
  }
  ORBFE_HIP_CHECK(hipGetLastError());
  return ORBFE_OK;
}
