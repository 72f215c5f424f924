// orbfe_init.hip -- Initializer on the GPU (include/orbfe_init.h): batched H/F RANSAC and
// reconstruction over the matches of several monocular bootstrap pairs.
//
//   k_init_normalize   one wavefront per frame: Normalize's float sums in key order
//   k_init_hypotheses  one thread per (hypothesis, model): selection + ComputeH21 / ComputeF21 + the
//                      composition; the Jacobi working set lane-interleaved in LDS
//   k_init_score       one wavefront per (hypothesis, model): the terms and inlier bits of 64 matches
//                      at a time in parallel, then the one float accumulator in match order
//   k_init_select      one thread per problem: the first best score of each model, RH, the branch and
//                      the 8 or 4 motion hypotheses
//   k_init_checkrt     one wavefront per motion hypothesis: CheckRT over the inliers, nGood and the
//                      selected cosine
//   k_init_decide      one block per problem: the gates up to the parallax, the candidate's vP3D /
//                      vbTriangulated
//
// One call stages every problem's inputs in one pinned buffer (one H2D copy), launches the kernels on
// the handle's stream and takes every result down in one D2H copy. All offsets into the buffers are
// formed on the host from counts it has checked against the handle's bounds; every index a kernel
// forms comes from a bounded loop, a host-checked draw or match, or an inlier bit below N.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/orbfe_init.h"
#include "orbfe_device.h"
#include "orbfe_init_core.h"
#include "orbfe_ktimer.h"
#include "orbfe_stage.h"

static_assert(INIT_FLAG_TOO_FEW == ORBFE_INIT_FLAG_TOO_FEW && INIT_FLAG_NO_MODEL == ORBFE_INIT_FLAG_NO_MODEL,
              "flag values");
static_assert(INIT_MODEL_H == ORBFE_INIT_MODEL_H && INIT_MODEL_F == ORBFE_INIT_MODEL_F, "model values");

#define INIT_HYP_THREADS 64

__device__ __forceinline__ float init_lane(float v, int l) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}

// acc + v[0] + v[1] + ... over the lanes whose bit is set in m, in lane order, one rounding each:
// every lane of the wavefront forms the same chain
__device__ __forceinline__ float init_chain(float acc, float v, unsigned long long m) {
#pragma unroll
  for (int l = 0; l < 64; l++) {
    const float x = init_lane(v, l);
    if ((m >> l) & 1ull) acc = acc + x;
  }
  return acc;
}

__global__ __launch_bounds__(128) void k_init_normalize(const uint8_t* __restrict__ in, uint8_t* __restrict__ res) {
  const InitDev& P = reinterpret_cast<const InitDev*>(in)[blockIdx.x];
  const int frame = threadIdx.x >> 6, lane = threadIdx.x & 63;  // wave-uniform
  const float* keys = reinterpret_cast<const float*>(in + (frame ? P.in_k2 : P.in_k1));
  const int n = frame ? P.n2 : P.n1;
  float mx = 0, my = 0;
  for (int c0 = 0; c0 < n; c0 += 64) {
    const int i = c0 + lane, cnt = n - c0;
    const unsigned long long m = cnt >= 64 ? ~0ull : (1ull << cnt) - 1ull;
    const float x = i < n ? keys[2 * (size_t)i] : 0.0f, y = i < n ? keys[2 * (size_t)i + 1] : 0.0f;
    mx = init_chain(mx, x, m);
    my = init_chain(my, y, m);
  }
  mx = mx / (float)n;
  my = my / (float)n;
  float dx = 0, dy = 0;
  for (int c0 = 0; c0 < n; c0 += 64) {
    const int i = c0 + lane, cnt = n - c0;
    const unsigned long long m = cnt >= 64 ? ~0ull : (1ull << cnt) - 1ull;
    const float x = i < n ? fabsf(keys[2 * (size_t)i] - mx) : 0.0f;
    const float y = i < n ? fabsf(keys[2 * (size_t)i + 1] - my) : 0.0f;
    dx = init_chain(dx, x, m);
    dy = init_chain(dy, y, m);
  }
  dx = dx / (float)n;
  dy = dy / (float)n;
  if (lane == 0) reinterpret_cast<InitNorm*>(res + P.o_nrm)[frame] = init_norm_of(mx, my, dx, dy);
}

// blockIdx.y: the model. The models land in the workspace: H21[n_hyp*9], H12[n_hyp*9], F21[n_hyp*9].
__global__ __launch_bounds__(INIT_HYP_THREADS) void k_init_hypotheses(const uint8_t* __restrict__ in,
                                                                      const uint8_t* __restrict__ res,
                                                                      uint8_t* __restrict__ ws) {
  const InitDev& P = reinterpret_cast<const InitDev*>(in)[blockIdx.z];
  __shared__ float sAt[INIT_WORK_AT * INIT_HYP_THREADS];
  __shared__ float sVt[INIT_WORK_VT * INIT_HYP_THREADS];
  __shared__ double sW[INIT_WORK_W * INIT_HYP_THREADS];
  const int k = blockIdx.x * INIT_HYP_THREADS + threadIdx.x;
  if (k >= P.n_hyp) return;  // no barrier below
  float* At = sAt + threadIdx.x;
  float* Vt = sVt + threadIdx.x;
  double* W = sW + threadIdx.x;
  const InitNorm* nrm = reinterpret_cast<const InitNorm*>(res + P.o_nrm);
  const InitNorm n1 = nrm[0], n2 = nrm[1];
  const int32_t* draw = reinterpret_cast<const int32_t*>(in + P.in_rand) + 8 * (size_t)k;
  int d[8], idx[8];
#pragma unroll
  for (int j = 0; j < 8; j++) d[j] = draw[j];  // checked by the host: 0 <= d[j] <= N-1-j
  init_select8(P.N, d, idx);
  const float* k1 = reinterpret_cast<const float*>(in + P.in_k1);
  const float* k2 = reinterpret_cast<const float*>(in + P.in_k2);
  const int32_t* m1 = reinterpret_cast<const int32_t*>(in + P.in_m1);
  const int32_t* m2 = reinterpret_cast<const int32_t*>(in + P.in_m2);
  float p1[16], p2[16];
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const size_t a = (size_t)m1[idx[j]], b = (size_t)m2[idx[j]];  // < n1, < n2: checked by the host
    init_norm_point(n1, k1[2 * a], k1[2 * a + 1], &p1[2 * j], &p1[2 * j + 1]);
    init_norm_point(n2, k2[2 * b], k2[2 * b + 1], &p2[2 * j], &p2[2 * j + 1]);
  }
  float T1[9], T2[9], M[9], TM[9], out[9];
  init_t_of(n1, T1);
  init_t_of(n2, T2);
  float* models = reinterpret_cast<float*>(ws + P.w_models);
  const size_t e = (size_t)P.n_hyp;
  if (blockIdx.y == INIT_MODEL_H) {
    float T2inv[9], H12[9];
    init_inv3(T2, T2inv);
    init_compute_h21(p1, p2, At, Vt, W, INIT_HYP_THREADS, M);
    init_gemm3(T2inv, M, TM);
    init_gemm3(TM, T1, out);
    init_inv3(out, H12);
#pragma unroll
    for (int i = 0; i < 9; i++) models[9 * (size_t)k + i] = out[i], models[9 * (e + k) + i] = H12[i];
  } else {
    float T2t[9];
    init_transpose3(T2, T2t);
    init_compute_f21(p1, p2, At, Vt, W, INIT_HYP_THREADS, M, nullptr);
    init_gemm3(T2t, M, TM);
    init_gemm3(TM, T1, out);
#pragma unroll
    for (int i = 0; i < 9; i++) models[9 * (2 * e + k) + i] = out[i];
  }
}

// blockIdx.x: the hypothesis, blockIdx.y: the model
__global__ __launch_bounds__(64) void k_init_score(const uint8_t* __restrict__ in, uint8_t* __restrict__ res,
                                                   uint8_t* __restrict__ ws) {
  const InitDev& P = reinterpret_cast<const InitDev*>(in)[blockIdx.z];
  const int k = blockIdx.x, lane = threadIdx.x;
  if (k >= P.n_hyp) return;  // block-uniform
  const bool is_h = blockIdx.y == INIT_MODEL_H;
  const float* models = reinterpret_cast<const float*>(ws + P.w_models);
  const size_t e = (size_t)P.n_hyp;
  float A[9], B[9];
#pragma unroll
  for (int i = 0; i < 9; i++) {
    A[i] = models[9 * ((is_h ? 0 : 2 * e) + k) + i];
    B[i] = is_h ? models[9 * (e + k) + i] : 0.0f;
  }
  const float* k1 = reinterpret_cast<const float*>(in + P.in_k1);
  const float* k2 = reinterpret_cast<const float*>(in + P.in_k2);
  const int32_t* m1 = reinterpret_cast<const int32_t*>(in + P.in_m1);
  const int32_t* m2 = reinterpret_cast<const int32_t*>(in + P.in_m2);
  unsigned long long* mask =
      reinterpret_cast<unsigned long long*>(ws + P.w_masks) + (size_t)P.words * ((is_h ? 0 : e) + k);
  const int N = P.N;
  float score = 0;
  for (int c0 = 0; c0 < N; c0 += 64) {  // c0 / 64 < words = ceil(N / 64)
    const int i = c0 + lane;
    bool in1 = false, in2 = false;
    float t1 = 0, t2 = 0;
    if (i < N) {
      const size_t a = (size_t)m1[i], b = (size_t)m2[i];
      const float u1 = k1[2 * a], v1 = k1[2 * a + 1], u2 = k2[2 * b], v2 = k2[2 * b + 1];
      if (is_h)
        init_check_h_match(A, B, u1, v1, u2, v2, P.inv_sigma2, &in1, &t1, &in2, &t2);
      else
        init_check_f_match(A, u1, v1, u2, v2, P.inv_sigma2, &in1, &t1, &in2, &t2);
    }
    const unsigned long long b1 = __ballot(in1), b2 = __ballot(in2);
#pragma unroll
    for (int l = 0; l < 64; l++) {  // two additions per match, in match order
      const float x1 = init_lane(t1, l), x2 = init_lane(t2, l);
      if ((b1 >> l) & 1ull) score = score + x1;
      if ((b2 >> l) & 1ull) score = score + x2;
    }
    if (lane == 0) mask[c0 >> 6] = b1 & b2;
  }
  if (lane == 0) reinterpret_cast<float*>(res + (is_h ? P.o_sh : P.o_sf))[k] = score;
}

__global__ __launch_bounds__(64) void k_init_select(const uint8_t* __restrict__ in, uint8_t* __restrict__ res,
                                                    const uint8_t* __restrict__ ws) {
  const InitDev& P = reinterpret_cast<const InitDev*>(in)[blockIdx.x];
  __shared__ float At[9], Vt[9];
  __shared__ double W[3];
  __shared__ int best[2];
  InitSel* S = reinterpret_cast<InitSel*>(res + P.o_sel);
  const float* models = reinterpret_cast<const float*>(ws + P.w_models);
  const size_t e = (size_t)P.n_hyp;
  if (threadIdx.x == 0) {
    const float* sh = reinterpret_cast<const float*>(res + P.o_sh);
    const float* sf = reinterpret_cast<const float*>(res + P.o_sf);
    float SH = 0, SF = 0;
    int bh = -1, bf = -1;
    for (int k = 0; k < P.n_hyp; k++) {  // currentScore > score: the first of equal scores stays
      if (sh[k] > SH) SH = sh[k], bh = k;
      if (sf[k] > SF) SF = sf[k], bf = k;
    }
    const float RH = SH / (SH + SF);
    const int model = (double)RH > 0.40 ? INIT_MODEL_H : INIT_MODEL_F;
    float H21[9], F21[9], K[9];
#pragma unroll
    for (int i = 0; i < 9; i++) {
      H21[i] = bh >= 0 ? models[9 * (size_t)bh + i] : 0.0f;
      F21[i] = bf >= 0 ? models[9 * (2 * e + bf) + i] : 0.0f;
      S->H21[i] = H21[i];
      S->F21[i] = F21[i];
    }
    init_k_matrix(P.k, K);
    unsigned flags = 0;
    int n_motions = 0;
    float R[72], t[24];
#pragma unroll
    for (int i = 0; i < 72; i++) R[i] = 0;
#pragma unroll
    for (int i = 0; i < 24; i++) t[i] = 0;
    if ((model == INIT_MODEL_H ? bh : bf) < 0) {
      flags |= INIT_FLAG_NO_MODEL;
    } else if (model == INIT_MODEL_H) {
      if (init_motions_h(H21, K, At, Vt, W, 1, R, t, nullptr)) n_motions = 8;
    } else {
      init_motions_f(F21, K, At, Vt, W, 1, R, t, nullptr);
      n_motions = 4;
    }
#pragma unroll
    for (int i = 0; i < 72; i++) S->R[i] = R[i];
#pragma unroll
    for (int i = 0; i < 24; i++) S->t[i] = t[i];
    S->best_h = bh, S->best_f = bf, S->model = model, S->n_motions = n_motions, S->candidate = -1;
    S->flags = flags;
    S->SH = SH, S->SF = SF, S->RH = RH;
#pragma unroll
    for (int j = 0; j < 8; j++) S->n_good[j] = 0, S->cosv[j] = 0;
    best[0] = bh, best[1] = bf;
  }
  __syncthreads();
  // the two winning masks, for the result and for k_init_checkrt
  const unsigned long long* masks = reinterpret_cast<const unsigned long long*>(ws + P.w_masks);
  unsigned long long* mh = reinterpret_cast<unsigned long long*>(res + P.o_mh);
  unsigned long long* mf = reinterpret_cast<unsigned long long*>(res + P.o_mf);
  for (int w = threadIdx.x; w < P.words; w += 64) {
    mh[w] = best[0] >= 0 ? masks[(size_t)P.words * best[0] + w] : 0ull;
    mf[w] = best[1] >= 0 ? masks[(size_t)P.words * (e + best[1]) + w] : 0ull;
  }
}

// blockIdx.x: the motion hypothesis
__global__ __launch_bounds__(64) void k_init_checkrt(const uint8_t* __restrict__ in, uint8_t* __restrict__ res,
                                                     uint8_t* __restrict__ ws) {
  const InitDev& P = reinterpret_cast<const InitDev*>(in)[blockIdx.y];
  InitSel* S = reinterpret_cast<InitSel*>(res + P.o_sel);
  const int j = blockIdx.x, lane = threadIdx.x;
  if (j >= S->n_motions) return;  // block-uniform
  const int n1 = P.n1, N = P.N;
  float* p3d = reinterpret_cast<float*>(ws + P.w_p3d) + 3 * (size_t)n1 * j;
  uint8_t* good = ws + P.w_good + (size_t)n1 * j;
  uint32_t* keys = reinterpret_cast<uint32_t*>(ws + P.w_cos) + (size_t)N * j;
  for (int i = lane; i < n1; i += 64) {  // vP3D.resize / vbGood = false over all of frame 1's keys
    p3d[3 * (size_t)i] = 0, p3d[3 * (size_t)i + 1] = 0, p3d[3 * (size_t)i + 2] = 0;
    good[i] = 0;
  }
  __threadfence_block();
  __syncthreads();
  float R[9], t[3], K[9], P2[12], O2[3], kk[4];
#pragma unroll
  for (int i = 0; i < 9; i++) R[i] = S->R[9 * j + i];
#pragma unroll
  for (int i = 0; i < 3; i++) t[i] = S->t[3 * j + i];
#pragma unroll
  for (int i = 0; i < 4; i++) kk[i] = P.k[i];
  init_k_matrix(kk, K);
  init_camera2(R, t, K, P2, O2);
  const unsigned long long* inl =
      reinterpret_cast<const unsigned long long*>(res + (S->model == INIT_MODEL_H ? P.o_mh : P.o_mf));
  const float* k1 = reinterpret_cast<const float*>(in + P.in_k1);
  const float* k2 = reinterpret_cast<const float*>(in + P.in_k2);
  const int32_t* m1 = reinterpret_cast<const int32_t*>(in + P.in_m1);
  const int32_t* m2 = reinterpret_cast<const int32_t*>(in + P.in_m2);
  int n_good = 0;
  for (int c0 = 0; c0 < N; c0 += 64) {
    const int i = c0 + lane;
    const unsigned long long word = inl[c0 >> 6];  // bits at or above N are 0
    bool pass = false, g = false;
    float X[3] = {0, 0, 0}, c = 0;
    size_t a = 0;
    if ((word >> lane) & 1ull) {
      a = (size_t)m1[i];
      const size_t b = (size_t)m2[i];
      pass = init_check_rt_match(R, t, P2, O2, kk, k1[2 * a], k1[2 * a + 1], k2[2 * b], k2[2 * b + 1], P.th2, X, &c, &g);
    }
    const unsigned long long pw = __ballot(pass);
    if (pass) {
      const int pos = n_good + __popcll(pw & ((1ull << lane) - 1ull));  // < N
      keys[pos] = init_order_key(c);
      p3d[3 * a] = X[0], p3d[3 * a + 1] = X[1], p3d[3 * a + 2] = X[2];  // a < n1, one match per key of frame 1
      good[a] = g ? 1 : 0;
    }
    n_good += __popcll(pw);
  }
  __threadfence_block();
  __syncthreads();
  float cosv = 0;
  if (n_good > 0) {
    // sort(vCosParallax)[min(50, size - 1)] by selection: the key's bits from the top, counting the
    // keys that share the prefix and have a 0 in this bit
    int r = n_good - 1 < 50 ? n_good - 1 : 50;
    uint32_t prefix = 0;
    for (int bit = 31; bit >= 0; bit--) {
      const uint32_t hi = bit == 31 ? 0u : (0xFFFFFFFFu << (bit + 1));
      int zeros = 0;
      for (int c0 = 0; c0 < n_good; c0 += 64) {
        const int i = c0 + lane;
        const uint32_t key = i < n_good ? keys[i] : 0u;
        const bool z = i < n_good && (key & hi) == (prefix & hi) && !((key >> bit) & 1u);
        zeros += __popcll(__ballot(z));
      }
      if (r >= zeros) {
        r -= zeros;
        prefix |= 1u << bit;
      }
    }
    cosv = init_key_value(prefix);
  }
  if (lane == 0) {
    S->n_good[j] = n_good;
    S->cosv[j] = cosv;
  }
}

__global__ __launch_bounds__(256) void k_init_decide(const uint8_t* __restrict__ in, uint8_t* __restrict__ res,
                                                     const uint8_t* __restrict__ ws) {
  const InitDev& P = reinterpret_cast<const InitDev*>(in)[blockIdx.x];
  InitSel* S = reinterpret_cast<InitSel*>(res + P.o_sel);
  __shared__ int cand;
  if (threadIdx.x == 0) {
    int c = -1, n_inl = 0;
    if (S->n_motions > 0) {
      const unsigned long long* inl =
          reinterpret_cast<const unsigned long long*>(res + (S->model == INIT_MODEL_H ? P.o_mh : P.o_mf));
      for (int w = 0; w < P.words; w++) n_inl += __popcll(inl[w]);
      int ng[8];
#pragma unroll
      for (int j = 0; j < 8; j++) ng[j] = S->n_good[j];
      c = S->model == INIT_MODEL_H ? init_decide_h(ng, n_inl) : init_decide_f(ng, n_inl);
    }
    S->candidate = c;
    S->n_inl = n_inl;
    cand = c;
  }
  __syncthreads();
  const int c = cand;  // < n_motions
  const int n1 = P.n1;
  float* op = reinterpret_cast<float*>(res + P.o_p3d);
  uint8_t* ot = res + P.o_tri;
  const float* p3d = reinterpret_cast<const float*>(ws + P.w_p3d) + 3 * (size_t)n1 * (c < 0 ? 0 : c);
  const uint8_t* good = ws + P.w_good + (size_t)n1 * (c < 0 ? 0 : c);
  for (int i = threadIdx.x; i < 3 * n1; i += 256) op[i] = c >= 0 ? p3d[i] : 0.0f;
  for (int i = threadIdx.x; i < n1; i += 256) ot[i] = c >= 0 ? good[i] : 0;
}

// ------------------------------------------------------------------------------------------
// host

struct orbfe_init : OrbfeDev {
  int S = 0, Kmax = 0, M = 0, H = 0;
  // inputs (one upload), results (one copy back), the workspace (device only); sized by init_plan_bounds
  OrbfeStage in, res, ws;
};

extern "C" int orbfe_init_create(int device, int max_problems, int max_keys, int max_matches, int max_hyp,
                                 orbfe_init** out) {
  if (!out) return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_init_create: bad argument");
  *out = nullptr;
  if (max_problems < 1 || max_problems > ORBFE_INIT_MAX_PROBLEMS || max_keys < 8 || max_keys > ORBFE_INIT_MAX_KEYS ||
      max_matches < 8 || max_matches > ORBFE_INIT_MAX_MATCHES || max_matches > max_keys || max_hyp < 1 ||
      max_hyp > ORBFE_INIT_MAX_HYP)
    return orbfe_set_error(ORBFE_ERR_ARG,
                           "orbfe_init_create: max_problems in 1..16, max_keys in 8..8192, max_matches in "
                           "8..min(8192, max_keys), max_hyp in 1..1024");
  orbfe_init* h = new orbfe_init();
  h->S = max_problems;
  h->Kmax = max_keys;
  h->M = max_matches;
  h->H = max_hyp;
  if (device < 0) {
    *out = h;
    return ORBFE_OK;
  }
  const int st = orbfe_dev_open(h, device, "orbfe_init_create");
  if (st != ORBFE_OK) {
    orbfe_init_destroy(h);
    return st;
  }
  size_t in_bytes, res_bytes, ws_bytes;
  init_plan_bounds(h->S, h->Kmax, h->M, h->H, &in_bytes, &res_bytes, &ws_bytes);
  ORBFE_CREATE_HIP(h, orbfe_init_destroy, orbfe_stage_alloc(&h->in, in_bytes, true));
  ORBFE_CREATE_HIP(h, orbfe_init_destroy, orbfe_stage_alloc(&h->res, res_bytes, true));
  ORBFE_CREATE_HIP(h, orbfe_init_destroy, orbfe_stage_alloc(&h->ws, ws_bytes, false));
  *out = h;
  return ORBFE_OK;
}

extern "C" int orbfe_init_destroy(orbfe_init* h) {
  if (!h) return ORBFE_OK;
  if (orbfe_dev_close(h)) {
    orbfe_stage_free(&h->in);
    orbfe_stage_free(&h->res);
    orbfe_stage_free(&h->ws);
  }
  delete h;
  return ORBFE_OK;
}

// Argument checks of one problem; *n_matches = N
static int init_check_problem(const orbfe_init* h, const orbfe_init_problem_t* p, const orbfe_init_result_t* r,
                              int* n_matches) {
  if (p->n1 < 1 || p->n2 < 1 || p->n_hyp < 0)
    return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_init_solve_batch: n1, n2 must be >= 1 and n_hyp >= 0");
  if (!p->keys1 || !p->keys2 || !p->matches12)
    return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_init_solve_batch: null keypoint or match array");
  if (!r->p3d || !r->triangulated)
    return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_init_solve_batch: null p3d or triangulated array");
  if (r->hyp_capacity < 0 || r->mask_words < 0)
    return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_init_solve_batch: bad result capacity");
  if (p->n1 > h->Kmax || p->n2 > h->Kmax)
    return orbfe_set_error(ORBFE_ERR_CAPACITY, "orbfe_init_solve_batch: keypoints above the handle's max_keys");
  if (p->n_hyp > h->H)
    return orbfe_set_error(ORBFE_ERR_CAPACITY, "orbfe_init_solve_batch: more hypotheses than the handle's max_hyp");
  int N = 0;
  for (int i = 0; i < p->n1; i++) {
    const int m = p->matches12[i];
    if (m >= p->n2) return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_init_solve_batch: matches12 entry >= n2");
    if (m >= 0) N++;
  }
  if (N > h->M)
    return orbfe_set_error(ORBFE_ERR_CAPACITY, "orbfe_init_solve_batch: matches above the handle's max_matches");
  *n_matches = N;
  if (((r->score_h || r->score_f) && p->n_hyp > r->hyp_capacity) ||
      ((r->mask_h || r->mask_f) && r->mask_words < (N + 63) / 64))
    return orbfe_set_error(ORBFE_ERR_CAPACITY, "orbfe_init_solve_batch: result capacity below n_hyp or ceil(N / 64)");
  if (N < 8) return ORBFE_OK;  // ORBFE_INIT_FLAG_TOO_FEW: not launched, the draws are not read
  if (p->n_hyp > 0 && !p->rand_idx) return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_init_solve_batch: null rand_idx");
  if (!ransac_check_draws(p->rand_idx, p->n_hyp, 8, N))
    return orbfe_set_error(ORBFE_ERR_ARG,
                           "orbfe_init_solve_batch: rand_idx outside 0 .. N-1-j for draw j of its iteration");
  return ORBFE_OK;
}

extern "C" int orbfe_init_solve_batch(orbfe_init* h, const orbfe_init_problem_t* problems, int n,
                                      orbfe_init_result_t* results) {
  if (!h || !problems || !results || n < 1)
    return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_init_solve_batch: bad argument");
  if (n > h->S)
    return orbfe_set_error(ORBFE_ERR_CAPACITY, "orbfe_init_solve_batch: more problems than the handle's max_problems");
  std::vector<int> N(n);
  for (int i = 0; i < n; i++) {
    const int st = init_check_problem(h, &problems[i], &results[i], &N[i]);
    if (st != ORBFE_OK) return st;
  }
  if (h->device < 0) return orbfe_set_error(ORBFE_ERR_STATE, "initializer is host-only (device < 0)");
  std::vector<int> act;
  for (int i = 0; i < n; i++)
    if (N[i] >= 8) act.push_back(i);
  const int na = (int)act.size();
  OrbfeStage &in = h->in, &res = h->res, &ws = h->ws;
  in.off = res.off = ws.off = 0;
  InitDev* dev;
  in.take<InitDev>((size_t)std::max(na, 1), &dev);
  int max_e = 0;
  for (int a = 0; a < na; a++) {
    const orbfe_init_problem_t& p = problems[act[a]];
    const size_t n1 = (size_t)p.n1, n2 = (size_t)p.n2, m = (size_t)N[act[a]], e = (size_t)p.n_hyp;
    InitDev d;
    memset(&d, 0, sizeof(d));
    d.n1 = p.n1, d.n2 = p.n2, d.N = (int)m, d.n_hyp = p.n_hyp, d.words = (int)((m + 63) / 64);
    for (int i = 0; i < 4; i++) d.k[i] = p.k[i];
    d.sigma = p.sigma;
    d.inv_sigma2 = (float)(1.0 / (double)(p.sigma * p.sigma));  // 1.0 / (sigma * sigma) (:335, :411)
    d.th2 = (float)(4.0 * (double)(p.sigma * p.sigma));         // 4.0 * mSigma2 into CheckRT's float th2
    init_layout(in, res, ws, n1, n2, m, e, d);
    if (in.off > in.cap || res.off > res.cap || ws.off > ws.cap)  // cannot happen within the bounds
      return orbfe_set_error(ORBFE_ERR_CAPACITY, "orbfe_init_solve_batch: staging plan exceeds the handle's buffers");
    memcpy(in.h + d.in_k1, p.keys1, 8 * n1);
    memcpy(in.h + d.in_k2, p.keys2, 8 * n2);
    int32_t* m1 = reinterpret_cast<int32_t*>(in.h + d.in_m1);
    int32_t* m2 = reinterpret_cast<int32_t*>(in.h + d.in_m2);
    size_t c = 0;
    for (int i = 0; i < p.n1; i++)  // mvMatches12 (:54-63)
      if (p.matches12[i] >= 0) m1[c] = i, m2[c] = p.matches12[i], c++;
    if (e) memcpy(in.h + d.in_rand, p.rand_idx, 32 * e);
    dev[a] = d;
    max_e = std::max(max_e, p.n_hyp);
  }
  if (na > 0) {
    ORBFE_HIP_CHECK(hipSetDevice(h->device));
    int st;
    if ((st = orbfe_stage_upload(&in, h->stream)) != ORBFE_OK) return st;
    const uint8_t* din = in.d;
    uint8_t* dres = res.d;
    uint8_t* dws = ws.d;
    ORBFE_LAUNCH("k_init_normalize", k_init_normalize, dim3(na), dim3(128), 0, h->stream, din, dres);
    if (max_e > 0) {
      ORBFE_LAUNCH("k_init_hypotheses", k_init_hypotheses,
                   dim3((max_e + INIT_HYP_THREADS - 1) / INIT_HYP_THREADS, 2, na), dim3(INIT_HYP_THREADS), 0,
                   h->stream, din, (const uint8_t*)dres, dws);
      ORBFE_LAUNCH("k_init_score", k_init_score, dim3(max_e, 2, na), dim3(64), 0, h->stream, din, dres, dws);
    }
    ORBFE_LAUNCH("k_init_select", k_init_select, dim3(na), dim3(64), 0, h->stream, din, dres, (const uint8_t*)dws);
    ORBFE_LAUNCH("k_init_checkrt", k_init_checkrt, dim3(8, na), dim3(64), 0, h->stream, din, dres, dws);
    ORBFE_LAUNCH("k_init_decide", k_init_decide, dim3(na), dim3(256), 0, h->stream, din, dres, (const uint8_t*)dws);
    if ((st = orbfe_stage_download(&res, h->stream)) != ORBFE_OK) return st;
  }
  for (int i = 0; i < n; i++) {
    orbfe_init_result_t& r = results[i];
    const orbfe_init_problem_t& p = problems[i];
    r.ok = 0;
    memset(r.r21, 0, sizeof(r.r21));
    memset(r.t21, 0, sizeof(r.t21));
    r.n_matches = N[i];
    r.flags = N[i] < 8 ? ORBFE_INIT_FLAG_TOO_FEW : 0u;
    r.sh = r.sf = r.rh = 0;
    r.model = ORBFE_INIT_MODEL_NONE;
    r.best_h = r.best_f = -1;
    memset(r.h21, 0, sizeof(r.h21));
    memset(r.f21, 0, sizeof(r.f21));
    r.n_motions = 0;
    memset(r.n_good, 0, sizeof(r.n_good));
    memset(r.cos_parallax, 0, sizeof(r.cos_parallax));
    r.candidate = r.motion = -1;
    r.parallax = 0;
    memset(r.p3d, 0, 12 * (size_t)p.n1);
    memset(r.triangulated, 0, (size_t)p.n1);
    if (r.score_h) memset(r.score_h, 0, 4 * (size_t)p.n_hyp);
    if (r.score_f) memset(r.score_f, 0, 4 * (size_t)p.n_hyp);
    if (r.mask_h) memset(r.mask_h, 0, 8 * (size_t)r.mask_words);
    if (r.mask_f) memset(r.mask_f, 0, 8 * (size_t)r.mask_words);
  }
  for (int a = 0; a < na; a++) {
    const InitDev& d = dev[a];
    orbfe_init_result_t& r = results[act[a]];
    const uint8_t* base = res.h;
    const InitSel& S = *reinterpret_cast<const InitSel*>(base + d.o_sel);
    const size_t e = (size_t)d.n_hyp;
    if (r.score_h) memcpy(r.score_h, base + d.o_sh, 4 * e);
    if (r.score_f) memcpy(r.score_f, base + d.o_sf, 4 * e);
    if (r.mask_h) orbfe_unpack_masks(r.mask_h, r.mask_words, base + d.o_mh, d.words, 1);
    if (r.mask_f) orbfe_unpack_masks(r.mask_f, r.mask_words, base + d.o_mf, d.words, 1);
    r.flags = S.flags;
    r.sh = S.SH, r.sf = S.SF, r.rh = S.RH;
    r.model = S.model;
    r.best_h = S.best_h, r.best_f = S.best_f;
    memcpy(r.h21, S.H21, sizeof(r.h21));
    memcpy(r.f21, S.F21, sizeof(r.f21));
    r.n_motions = S.n_motions;
    memcpy(r.n_good, S.n_good, sizeof(r.n_good));
    memcpy(r.cos_parallax, S.cosv, sizeof(r.cos_parallax));
    r.candidate = S.candidate;
    if (S.candidate < 0) continue;
    // acos(c) * 180 / CV_PI (:978) on the host. LIBM: std::acos(float) is acosf
    const float c = S.cosv[S.candidate];
    r.parallax = S.n_good[S.candidate] > 0 ? (float)((double)(acosf(c) * 180.0f) / 3.1415926535897932384626433832795)
                                            : 0.0f;
    const float min_parallax = problems[act[a]].min_parallax;
    r.ok = S.model == INIT_MODEL_H ? r.parallax >= min_parallax : r.parallax > min_parallax;  // :786, :572
    if (!r.ok) continue;
    r.motion = S.candidate;
    memcpy(r.r21, S.R + 9 * r.motion, sizeof(r.r21));
    memcpy(r.t21, S.t + 3 * r.motion, sizeof(r.t21));
    memcpy(r.p3d, base + d.o_p3d, 12 * (size_t)d.n1);
    memcpy(r.triangulated, base + d.o_tri, (size_t)d.n1);
  }
  return ORBFE_OK;
}
