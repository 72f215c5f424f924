// orbfe_lm_device.h -- the wavefront group of the in-kernel Levenberg-Marquardt solvers (k_poseopt,
// k_optsim3): the device's counterpart of orbfe_lm_core.h's PoHostGroup. Device code only.
#pragma once
#include "orbfe_lm_core.h"

struct LmDevGroup {
  static constexpr int width = PO_LANES;
  static constexpr int slots = 1;
  __device__ int lane() const { return threadIdx.x; }
  __device__ void sync() const { __syncthreads(); }  // the block is one wavefront
  double* red;  // LDS, as many doubles as the widest reduce<N> of the caller
  // The tree: after the step of `stride` lanes 0 .. stride-1 hold s[l] + s[l + stride]. Lane 0's sums go
  // to every lane through LDS, which keeps them in vector registers: as wave-uniform values the
  // Levenberg state would not fit the scalar register file.
  template <int N>
  __device__ void reduce(double (*s)[N]) const {
    __syncthreads();  // every lane has read the previous sums
#pragma unroll
    for (int k = 0; k < N; k++) {
      double v = s[0][k];
#pragma unroll
      for (int stride = PO_LANES / 2; stride >= 1; stride >>= 1) v = v + __shfl_down(v, stride);
      if (threadIdx.x == 0) red[k] = v;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; k++) s[0][k] = red[k];
  }
  __device__ uint64_t ballot(const uint64_t* bits, int c) const { return __ballot((int)((bits[0] >> c) & 1ull)); }
};
