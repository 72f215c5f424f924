// orbfe_gridmap.hip -- the occupancy grid on gfx950 (include/orbfe_gridmap.h): UpdateGridMap of any
// number of keyframes as one batch of beams, BuildOccupancyGridMsg as a streaming pass.
//
// Reference: src/GridMapping.cpp:72-154, 176-181, 232-270. orbfe_gridmap_core.h holds every rule; the
// kernels below only distribute the work.
//
// A call is worked off in groups of whole keyframes of at most GM_GROUP points. Per group:
//   k_gm_gather   (resident only) one workgroup per keyframe: the row's live points, in slot order, from
//                 the geometry store into the group's position array (ballot compaction, 256 slots a pass).
//   k_gm_cells    one workgroup per keyframe, 2048 points a tile: the cells of the points, the first
//                 outside point (REFERENCE: the keyframe ends there), the start of every beam -- under
//                 REFERENCE rules lane 0 replays CastLaserBeam's swaps serially over the tile's cells in
//                 LDS (integer only, no grid traffic) -- the occupied increments, and per beam its record
//                 (start, end) and its number of segments.
//   then, over sub-ranges of at most seg_cap / ceil(max(rows, cols) / SEGMENT) beams (so that a
//   sub-range's segments always fit the segment arrays):
//   k_gm_scan_*   exclusive scan of the segment counts (1024 per workgroup, one workgroup over the tops).
//   k_gm_walk     one lane per beam, no memory traffic but the records: replays the double error with
//                 gm_beam_step and stores (x, y, error) at every SEGMENT-th step.
//   k_gm_scatter  one lane per segment: at most SEGMENT steps of gm_beam_step from the stored state, one
//                 no-return atomicAdd per visited cell. Lanes beyond the scanned total leave at once (the
//                 launch is sized for the worst case, so no count comes back to the host between passes).
// Tallies (beams, visits, dropped writes, touched rows, ...) are summed per wavefront and added with one
// atomic per wavefront. k_gm_build: four cells per lane, two 16-byte loads and one dword store.
// Guards: a keyframe against the group's count, a point against its keyframe's region and the group's
// capacity, a row against M, a slot against S and the row's length, a point id against P, a segment offset
// against seg_cap, a flat index against rows * cols (gm_visit_index), a dword against the padded cell count.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstring>
#include <vector>

#include "../../include/orbfe.h"
#include "../../include/orbfe_gridmap.h"
#include "orbfe_covis_view.h"
#include "orbfe_device.h"
#include "orbfe_gridmap_core.h"
#include "orbfe_ktimer.h"
#include "orbfe_localmap_core.h"
#include "orbfe_stage.h"

namespace lm = orbfe_localmap_core;

#define GM_THREADS 256
#define GM_TILE 2048                 // points per tile of k_gm_cells
#define GM_GROUP (1 << 18)           // points per group of keyframes
#define GM_SEG_CAP (1 << 22)         // segments per sub-range, at least
#define GM_SCAN_TILE 1024            // entries per workgroup of the scan
#define GM_PROB_CHUNK (1 << 22)      // floats of the probability staging
#define GM_S ORBFE_GRIDMAP_SEGMENT

static_assert(GM_GROUP >= ORBFE_GRIDMAP_MAX_POINTS, "a group holds at least one keyframe");
static_assert(GM_GROUP <= GM_SCAN_TILE * GM_SCAN_TILE, "the scan's second level is one workgroup");
static_assert(ORBFE_GRIDMAP_MAX_KEYFRAMES == lm::kMaxList, "update_resident shares the covisibility list bound");

enum { GM_ST_BEAMS, GM_ST_VISITS, GM_ST_DROPPED, GM_ST_CUT, GM_ST_KF_OUT, GM_ST_MISSING, GM_ST_ROW_MIN, GM_ST_ROW_MAX, GM_ST_N };

struct GmArgs {
  GmGrid g;
  int rules;
  int32_t* occupied;
  int32_t* visits;
  // the group
  int n_kf;                  // keyframes of the group
  int n_pts;                 // points (padded regions) of the group, <= GM_GROUP
  const float* centres;      // [n_kf * 3]
  const int32_t* kf_begin;   // [n_kf] region start within the group
  const int32_t* kf_len;     // [n_kf] region length
  int32_t* kf_count;         // [n_kf] points in the region (gather writes it; <= kf_len)
  float* pos;                // [GM_GROUP * 3]
  int4* rec;                 // [GM_GROUP] start x, start z, point x, point z (point x < 0: no beam)
  int32_t* seg;              // [GM_GROUP] segments per beam, then offsets within a sub-range
  // the segments of a sub-range
  int2* seg_xy;
  double* seg_err;
  int32_t* seg_beam;
  int seg_cap;
  int32_t* total;            // the scanned total of the current sub-range
  long long* stat;           // [GM_ST_N]
};

__device__ __forceinline__ void gm_stat_add(long long* stat, int which, int v) {
  const int s = wave_sum(v);
  if (lane_id() == 0 && s != 0) atomicAdd((unsigned long long*)&stat[which], (unsigned long long)s);
}
__device__ __forceinline__ void gm_stat_rows(long long* stat, int lo, int hi) {
  lo = wave_min(lo);
  hi = wave_max(hi);
  if (lane_id() == 0 && hi >= 0) {
    atomicMin(&stat[GM_ST_ROW_MIN], (long long)lo);
    atomicMax(&stat[GM_ST_ROW_MAX], (long long)hi);
  }
}

__global__ void k_gm_stat_init(long long* stat) {
  const int i = threadIdx.x;
  if (i < GM_ST_N) stat[i] = i == GM_ST_ROW_MIN ? (long long)INT_MAX : i == GM_ST_ROW_MAX ? -1ll : 0ll;
}

struct GmRows {
  const int32_t* rows;
  const int32_t* row_n;
  const uint8_t* bad;
  const uint8_t* rec;
  const uint8_t* state;
  int M, S, P;
  const int32_t* list_rows;  // [n_kf] of the call / of the group
};

// the live point in slot s of list position k, or -1
__device__ __forceinline__ int gm_slot_point(const GmRows& r, int k, int s) {
  const int row = r.list_rows[k];
  if ((unsigned)row >= (unsigned)r.M) return -1;
  if (s >= r.row_n[row] || s >= r.S) return -1;
  const int p = r.rows[(size_t)row * r.S + s];
  if ((unsigned)p >= (unsigned)r.P) return -1;
  return r.bad[p] ? -1 : p;
}

// grid (slot blocks, n_kf): live points whose geometry was never set
__global__ __launch_bounds__(GM_THREADS) void k_gm_missing(GmRows r, long long* stat) {
  const int s = (int)(blockIdx.x * GM_THREADS + threadIdx.x);
  const int p = gm_slot_point(r, blockIdx.y, s);
  const int miss = p >= 0 && (!r.state || !(r.state[p] & lm::kPresent)) ? 1 : 0;
  gm_stat_add(stat, GM_ST_MISSING, miss);
}

// grid n_kf: the live points of a row, in slot order, into the keyframe's region of pos
__global__ __launch_bounds__(GM_THREADS) void k_gm_gather(GmRows r, GmArgs a) {
  __shared__ int s_w[GM_THREADS / 64];
  const int k = blockIdx.x;
  if (k >= a.n_kf) return;
  const int base = a.kf_begin[k], len = a.kf_len[k];
  const int w = wave_id();
  int run = 0;
  for (int t = 0; t < len; t += GM_THREADS) {
    const int s = t + (int)threadIdx.x;
    int p = s < len ? gm_slot_point(r, k, s) : -1;
    if (p >= 0 && !(r.state[p] & lm::kPresent)) p = -1;  // k_gm_missing has refused the call before this
    const uint64_t m = wave_ballot(p >= 0);
    if (lane_id() == 0) s_w[w] = __popcll(m);
    __syncthreads();
    int off = run, tot = 0;
    for (int q = 0; q < GM_THREADS / 64; q++) {
      off += q < w ? s_w[q] : 0;
      tot += s_w[q];
    }
    const int idx = off + prefix_in_wave(m);
    if (p >= 0 && idx < len && base + idx < GM_GROUP) {
      const float* src = reinterpret_cast<const float*>(r.rec + (size_t)p * lm::kRecord + 32);
      float* dst = a.pos + 3 * (size_t)(base + idx);
      dst[0] = src[0];
      dst[1] = src[1];
      dst[2] = src[2];
    }
    run += tot;
    __syncthreads();  // s_w is written again
  }
  if (threadIdx.x == 0) a.kf_count[k] = min(run, len);
}

// grid n_kf
__global__ __launch_bounds__(GM_THREADS) void k_gm_cells(GmArgs a) {
  __shared__ int2 s_cell[GM_TILE];
  __shared__ int2 s_start[GM_TILE];
  __shared__ int s_first;
  __shared__ int s_state[2];
  const int k = blockIdx.x, tid = threadIdx.x;
  if (k >= a.n_kf) return;
  const GmGrid g = a.g;
  const bool chained = a.rules == ORBFE_GRIDMAP_REFERENCE;
  const int base = a.kf_begin[k], len = a.kf_len[k], n = min(a.kf_count[k], len);
  const int kx = gm_cell(a.centres[3 * k], g.scale, g.min_x, g.norm_x, g.cols);
  const int kz = gm_cell(a.centres[3 * k + 2], g.scale, g.min_z, g.norm_z, g.rows);
  const bool kf_out = kx < 0 || kz < 0;
  if (tid == 0) {
    s_state[0] = kx;
    s_state[1] = kz;
    if (kf_out) atomicAdd((unsigned long long*)&a.stat[GM_ST_KF_OUT], 1ull);
  }
  bool done = kf_out;  // uniform: no further point of this keyframe is cast
  int beams = 0, cut = 0, row_lo = INT_MAX, row_hi = -1;
  for (int t0 = 0; t0 < len; t0 += GM_TILE) {
    const int tn = min(GM_TILE, len - t0);
    if (tid == 0) s_first = GM_TILE;
    __syncthreads();
    for (int j = tid; j < tn; j += GM_THREADS) {
      const int i = t0 + j;
      int px = -1, pz = -1;
      if (!done && i < n && base + i < GM_GROUP) {
        const float* p = a.pos + 3 * (size_t)(base + i);
        px = gm_cell(p[0], g.scale, g.min_x, g.norm_x, g.cols);
        pz = gm_cell(p[2], g.scale, g.min_z, g.norm_z, g.rows);
        if (px < 0 || pz < 0) {
          px = pz = -1;
          if (chained)
            atomicMin(&s_first, j);
          else
            cut++;
        }
      }
      s_cell[j] = make_int2(px, pz);
    }
    __syncthreads();
    const int first = s_first;
    // the tile's points that are cast form a prefix under REFERENCE rules
    const int nv = done ? 0 : min(min(first, tn), max(n - t0, 0));
    if (chained && tid == 0) {
      if (!done && first < GM_TILE) cut += n - (t0 + first);
      int cx = s_state[0], cz = s_state[1];
      for (int j = 0; j < nv; j++) {
        int2 c = s_cell[j];
        s_start[j] = make_int2(cx, cz);
        gm_beam_swaps(cx, cz, c.x, c.y);
      }
      s_state[0] = cx;
      s_state[1] = cz;
    }
    __syncthreads();
    for (int j = tid; j < tn; j += GM_THREADS) {
      const int i = t0 + j;
      if (base + i >= GM_GROUP) continue;
      const int2 c = s_cell[j];
      const bool cast = c.x >= 0 && (!chained || j < nv);
      int4 rec = make_int4(0, 0, -1, -1);
      int nseg = 0;
      if (cast) {
        int sx = chained ? s_start[j].x : kx, sz = chained ? s_start[j].y : kz;
        rec = make_int4(sx, sz, c.x, c.y);
        atomicAdd(&a.occupied[(size_t)c.y * g.cols + c.x], 1);
        row_lo = min(row_lo, c.y);
        row_hi = max(row_hi, c.y);
        const GmBeam b = gm_beam_setup(sx, sz, c.x, c.y);
        nseg = (gm_beam_steps(b) + GM_S - 1) / GM_S;
        beams++;
      }
      a.rec[base + i] = rec;
      a.seg[base + i] = nseg;
    }
    if (chained && first < GM_TILE) done = true;
  }
  gm_stat_add(a.stat, GM_ST_BEAMS, beams);
  gm_stat_add(a.stat, GM_ST_CUT, cut);
  gm_stat_rows(a.stat, row_lo, row_hi);
}

// Exclusive scan of data[0..n): 1024 entries per workgroup, the workgroup's total to tops.
__device__ __forceinline__ int gm_block_scan4(int (&v)[4], int* s_wsum) {
  const int lane = lane_id(), w = wave_id();
  const int s = v[0] + v[1] + v[2] + v[3];
  int inc = s;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_up(inc, o, 64);
    if (lane >= o) inc += y;
  }
  if (lane == 63) s_wsum[w] = inc;
  __syncthreads();
  int off = 0, total = 0;
#pragma unroll
  for (int q = 0; q < GM_THREADS / 64; q++) {
    const int x = s_wsum[q];
    off += q < w ? x : 0;
    total += x;
  }
  int run = off + inc - s;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int x = v[j];
    v[j] = run;
    run += x;
  }
  return total;
}
__global__ __launch_bounds__(GM_THREADS) void k_gm_scan_local(int32_t* data, int n, int32_t* tops) {
  __shared__ int s_wsum[GM_THREADS / 64];
  const int base = (int)blockIdx.x * GM_SCAN_TILE + (int)threadIdx.x * 4;
  int v[4];
#pragma unroll
  for (int j = 0; j < 4; j++) v[j] = base + j < n ? data[base + j] : 0;
  const int total = gm_block_scan4(v, s_wsum);
#pragma unroll
  for (int j = 0; j < 4; j++)
    if (base + j < n) data[base + j] = v[j];
  if (threadIdx.x == 0) tops[blockIdx.x] = total;
}
__global__ __launch_bounds__(GM_THREADS) void k_gm_scan_tops(int32_t* tops, int nb, int32_t* total_out) {
  __shared__ int s_wsum[GM_THREADS / 64];
  const int base = (int)threadIdx.x * 4;
  int v[4];
#pragma unroll
  for (int j = 0; j < 4; j++) v[j] = base + j < nb ? tops[base + j] : 0;
  const int total = gm_block_scan4(v, s_wsum);
#pragma unroll
  for (int j = 0; j < 4; j++)
    if (base + j < nb) tops[base + j] = v[j];
  if (threadIdx.x == 0) *total_out = total;
}
__global__ __launch_bounds__(GM_THREADS) void k_gm_scan_add(int32_t* data, int n, const int32_t* tops) {
  const int add = tops[blockIdx.x];
  const int base = (int)blockIdx.x * GM_SCAN_TILE + (int)threadIdx.x * 4;
#pragma unroll
  for (int j = 0; j < 4; j++)
    if (base + j < n) data[base + j] += add;
}

// one lane per beam of [b0, b1): the state at the start of each of its segments
__global__ __launch_bounds__(GM_THREADS) void k_gm_walk(GmArgs a, int b0, int b1) {
  const int i = b0 + (int)(blockIdx.x * GM_THREADS + threadIdx.x);
  if (i >= b1 || i >= a.n_pts) return;
  const int4 r = a.rec[i];
  if (r.z < 0) return;
  int sx = r.x, sz = r.y;
  const GmBeam b = gm_beam_setup(sx, sz, r.z, r.w);
  const int nseg = (gm_beam_steps(b) + GM_S - 1) / GM_S;
  const int off = a.seg[i];
  if (off < 0 || off > a.seg_cap - nseg) return;
  double error = 0;
  int y = b.y, x = b.x;
  for (int s = 0; s < nseg; s++) {
    a.seg_xy[off + s] = make_int2(x, y);
    a.seg_err[off + s] = error;
    a.seg_beam[off + s] = i;
    if (s + 1 == nseg) break;
    for (int q = 0; q < GM_S; q++) gm_beam_step(y, error, b.deltaerr, b.ystep);
    x += GM_S;
  }
}

// one lane per segment of the current sub-range
__global__ __launch_bounds__(GM_THREADS) void k_gm_scatter(GmArgs a) {
  const long long t = (long long)blockIdx.x * GM_THREADS + threadIdx.x;
  const int total = min(*a.total, a.seg_cap);
  int visits = 0, dropped = 0, row_lo = INT_MAX, row_hi = -1;
  if (t < total) {
    const int i = a.seg_beam[t];
    if ((unsigned)i < (unsigned)a.n_pts) {
      const int4 r = a.rec[i];
      int sx = r.x, sz = r.y;
      const GmBeam b = gm_beam_setup(sx, sz, r.z, r.w);
      const int2 xy = a.seg_xy[t];
      double error = a.seg_err[t];
      int y = xy.y;
      const int xe = min(b.x1, xy.x + GM_S - 1);
      const int rows = a.g.rows, cols = a.g.cols;
      for (int x = xy.x; x <= xe; ++x) {
        const long long flat = gm_visit_index(x, y, b.steep, rows, cols);
        if (flat < 0) {
          dropped++;
        } else {
          atomicAdd(&a.visits[flat], 1);
          visits++;
          const int col = b.steep ? y : x;
          int row = b.steep ? x : y;
          if (col >= cols) row += col / cols;  // the write wrapped into a later row
          row_lo = min(row_lo, row);
          row_hi = max(row_hi, row);
        }
        gm_beam_step(y, error, b.deltaerr, b.ystep);
      }
    }
  }
  gm_stat_add(a.stat, GM_ST_VISITS, visits);
  gm_stat_add(a.stat, GM_ST_DROPPED, dropped);
  gm_stat_rows(a.stat, row_lo, row_hi);
}

// dwords [d0, d1) of the grid: cells 4d .. 4d + 3 (the arrays are padded to a multiple of four cells)
__global__ __launch_bounds__(GM_THREADS) void k_gm_build(const int4* occupied, const int4* visits, uint32_t* grid,
                                                         long long d0, long long d1, int visit_threshold) {
  const long long d = d0 + (long long)blockIdx.x * GM_THREADS + threadIdx.x;
  if (d >= d1) return;
  const int4 v = visits[d], o = occupied[d];
  const uint32_t m0 = (uint8_t)gm_cell_msg(gm_cell_data(o.x, v.x, visit_threshold));
  const uint32_t m1 = (uint8_t)gm_cell_msg(gm_cell_data(o.y, v.y, visit_threshold));
  const uint32_t m2 = (uint8_t)gm_cell_msg(gm_cell_data(o.z, v.z, visit_threshold));
  const uint32_t m3 = (uint8_t)gm_cell_msg(gm_cell_data(o.w, v.w, visit_threshold));
  grid[d] = m0 | (m1 << 8) | (m2 << 16) | (m3 << 24);
}

// cells [c0, c0 + n) of the float data grid into out[0..n)
__global__ __launch_bounds__(GM_THREADS) void k_gm_probability(const int32_t* occupied, const int32_t* visits,
                                                               long long c0, int n, int visit_threshold, float* out) {
  const int i = (int)(blockIdx.x * GM_THREADS + threadIdx.x);
  if (i >= n) return;
  out[i] = gm_cell_data(occupied[c0 + i], visits[c0 + i], visit_threshold);
}

// ------------------------------------------------------------------------------------------
// host

struct orbfe_gridmap : OrbfeDev {
  int rules = ORBFE_GRIDMAP_REFERENCE;
  GmGrid g{};
  long long cells = 0, cells_pad = 0;
  int spb = 1;      // segments of the longest beam
  int seg_cap = 0;  // entries of the segment arrays
  int sub = 0;      // beams per sub-range
  int32_t* d_occupied = nullptr;
  int32_t* d_visits = nullptr;
  int8_t* d_grid = nullptr;
  float* d_pos = nullptr;
  int4* d_rec = nullptr;
  int32_t* d_seg = nullptr;
  int2* d_seg_xy = nullptr;
  double* d_seg_err = nullptr;
  int32_t* d_seg_beam = nullptr;
  int32_t* d_tops = nullptr;      // [GM_SCAN_TILE + 1]: the tops, then the total
  float* d_centres = nullptr;     // [4096 * 3]
  int32_t* d_kf = nullptr;        // [4 * 4096]: begin, len, count, list rows
  long long* d_stat = nullptr;    // [GM_ST_N]
  long long* h_stat = nullptr;    // pinned
  float* d_prob = nullptr;        // [GM_PROB_CHUNK]
  int dirty0 = 0, dirty1 = 0;     // rows an increment touched since the last build
  std::vector<int32_t> kf_begin, kf_len, list_rows, row_len;
};

static const char* const kGmHostOnly = "the grid is host-only (device < 0)";

extern "C" int orbfe_gridmap_create(int device, const orbfe_gridmap_geometry* geo, int rules, orbfe_gridmap** out) {
  if (!out) return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_gridmap_create: bad argument");
  *out = nullptr;
  GmGrid g;
  const int gs = gm_grid_of(geo, &g);
  if (gs) return orbfe_set_error(gs, "orbfe_gridmap_create: bad geometry");
  if (rules != ORBFE_GRIDMAP_REFERENCE && rules != ORBFE_GRIDMAP_INTENDED)
    return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_gridmap_create: unknown rules");
  orbfe_gridmap* h = new orbfe_gridmap();
  h->g = g;
  h->rules = rules;
  h->cells = (long long)g.rows * g.cols;
  h->cells_pad = (h->cells + 3) & ~3ll;
  h->spb = (std::max(g.rows, g.cols) + GM_S - 1) / GM_S;
  h->seg_cap = std::max(GM_SEG_CAP, h->spb);
  h->sub = std::max(1, std::min(GM_GROUP, h->seg_cap / h->spb));
  if (device < 0) {
    *out = h;
    return ORBFE_OK;
  }
  const int open_st = orbfe_dev_open(h, device, "orbfe_gridmap_create");
  if (open_st != ORBFE_OK) {
    orbfe_gridmap_destroy(h);
    return open_st;
  }
  const size_t pad = (size_t)h->cells_pad, cap = (size_t)h->seg_cap;
  ORBFE_CREATE_HIP(h, orbfe_gridmap_destroy, hipMalloc((void**)&h->d_occupied, 4 * pad));
  ORBFE_CREATE_HIP(h, orbfe_gridmap_destroy, hipMalloc((void**)&h->d_visits, 4 * pad));
  ORBFE_CREATE_HIP(h, orbfe_gridmap_destroy, hipMalloc((void**)&h->d_grid, pad));
  ORBFE_CREATE_HIP(h, orbfe_gridmap_destroy, hipMalloc((void**)&h->d_pos, 12 * (size_t)GM_GROUP));
  ORBFE_CREATE_HIP(h, orbfe_gridmap_destroy, hipMalloc((void**)&h->d_rec, 16 * (size_t)GM_GROUP));
  ORBFE_CREATE_HIP(h, orbfe_gridmap_destroy, hipMalloc((void**)&h->d_seg, 4 * (size_t)GM_GROUP));
  ORBFE_CREATE_HIP(h, orbfe_gridmap_destroy, hipMalloc((void**)&h->d_seg_xy, 8 * cap));
  ORBFE_CREATE_HIP(h, orbfe_gridmap_destroy, hipMalloc((void**)&h->d_seg_err, 8 * cap));
  ORBFE_CREATE_HIP(h, orbfe_gridmap_destroy, hipMalloc((void**)&h->d_seg_beam, 4 * cap));
  ORBFE_CREATE_HIP(h, orbfe_gridmap_destroy, hipMalloc((void**)&h->d_tops, 4 * (GM_SCAN_TILE + 1)));
  ORBFE_CREATE_HIP(h, orbfe_gridmap_destroy, hipMalloc((void**)&h->d_centres, 12 * (size_t)ORBFE_GRIDMAP_MAX_KEYFRAMES));
  ORBFE_CREATE_HIP(h, orbfe_gridmap_destroy, hipMalloc((void**)&h->d_kf, 16 * (size_t)ORBFE_GRIDMAP_MAX_KEYFRAMES));
  ORBFE_CREATE_HIP(h, orbfe_gridmap_destroy, hipMalloc((void**)&h->d_stat, 8 * GM_ST_N));
  ORBFE_CREATE_HIP(h, orbfe_gridmap_destroy, hipHostMalloc((void**)&h->h_stat, 8 * GM_ST_N, hipHostMallocDefault));
  ORBFE_CREATE_HIP(h, orbfe_gridmap_destroy, hipMalloc((void**)&h->d_prob, 4 * (size_t)GM_PROB_CHUNK));
  ORBFE_CREATE_HIP(h, orbfe_gridmap_destroy, hipMemsetAsync(h->d_occupied, 0, 4 * pad, h->stream));
  ORBFE_CREATE_HIP(h, orbfe_gridmap_destroy, hipMemsetAsync(h->d_visits, 0, 4 * pad, h->stream));
  ORBFE_CREATE_HIP(h, orbfe_gridmap_destroy, hipMemsetAsync(h->d_grid, 0, pad, h->stream));
  ORBFE_CREATE_HIP(h, orbfe_gridmap_destroy, hipStreamSynchronize(h->stream));
  *out = h;
  return ORBFE_OK;
}

extern "C" int orbfe_gridmap_destroy(orbfe_gridmap* h) {
  if (!h) return ORBFE_OK;
  if (orbfe_dev_close(h)) {
    hipFree(h->d_occupied);
    hipFree(h->d_visits);
    hipFree(h->d_grid);
    hipFree(h->d_pos);
    hipFree(h->d_rec);
    hipFree(h->d_seg);
    hipFree(h->d_seg_xy);
    hipFree(h->d_seg_err);
    hipFree(h->d_seg_beam);
    hipFree(h->d_tops);
    hipFree(h->d_centres);
    hipFree(h->d_kf);
    hipFree(h->d_stat);
    hipFree(h->d_prob);
    if (h->h_stat) hipHostFree(h->h_stat);
  }
  delete h;
  return ORBFE_OK;
}

extern "C" int orbfe_gridmap_reset(orbfe_gridmap* h) {
  if (!h) return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_gridmap_reset: bad argument");
  if (h->device < 0) return orbfe_set_error(ORBFE_ERR_STATE, kGmHostOnly);
  hipSetDevice(h->device);
  const size_t pad = (size_t)h->cells_pad;
  ORBFE_HIP_CHECK(hipMemsetAsync(h->d_occupied, 0, 4 * pad, h->stream));
  ORBFE_HIP_CHECK(hipMemsetAsync(h->d_visits, 0, 4 * pad, h->stream));
  ORBFE_HIP_CHECK(hipMemsetAsync(h->d_grid, 0, pad, h->stream));
  ORBFE_HIP_CHECK(hipStreamSynchronize(h->stream));
  h->dirty0 = h->dirty1 = 0;
  return ORBFE_OK;
}

static GmArgs gm_args(orbfe_gridmap* h) {
  GmArgs a;
  a.g = h->g;
  a.rules = h->rules;
  a.occupied = h->d_occupied;
  a.visits = h->d_visits;
  a.n_kf = 0;
  a.n_pts = 0;
  a.centres = h->d_centres;
  a.kf_begin = h->d_kf;
  a.kf_len = h->d_kf + ORBFE_GRIDMAP_MAX_KEYFRAMES;
  a.kf_count = h->d_kf + 2 * ORBFE_GRIDMAP_MAX_KEYFRAMES;
  a.pos = h->d_pos;
  a.rec = h->d_rec;
  a.seg = h->d_seg;
  a.seg_xy = h->d_seg_xy;
  a.seg_err = h->d_seg_err;
  a.seg_beam = h->d_seg_beam;
  a.seg_cap = h->seg_cap;
  a.total = h->d_tops + GM_SCAN_TILE;
  a.stat = h->d_stat;
  return a;
}

// The passes of one group whose keyframe arrays (and positions, or rows) are on the device. Returns with
// the stream idle, so that the caller may refill the group's arrays.
static int gm_run_group(orbfe_gridmap* h, GmArgs a, const GmRows* rows) {
  const dim3 block(GM_THREADS);
  if (rows) ORBFE_LAUNCH("k_gm_gather", k_gm_gather, dim3(a.n_kf), block, 0, h->stream, *rows, a);
  ORBFE_LAUNCH("k_gm_cells", k_gm_cells, dim3(a.n_kf), block, 0, h->stream, a);
  for (int b0 = 0; b0 < a.n_pts; b0 += h->sub) {
    const int b1 = std::min(a.n_pts, b0 + h->sub), n = b1 - b0;
    const int nb = (n + GM_SCAN_TILE - 1) / GM_SCAN_TILE;
    ORBFE_LAUNCH("k_gm_scan_local", k_gm_scan_local, dim3(nb), block, 0, h->stream, a.seg + b0, n, h->d_tops);
    ORBFE_LAUNCH("k_gm_scan_tops", k_gm_scan_tops, dim3(1), block, 0, h->stream, h->d_tops, nb, a.total);
    ORBFE_LAUNCH("k_gm_scan_add", k_gm_scan_add, dim3(nb), block, 0, h->stream, a.seg + b0, n, (const int32_t*)h->d_tops);
    ORBFE_LAUNCH("k_gm_walk", k_gm_walk, dim3((n + GM_THREADS - 1) / GM_THREADS), block, 0, h->stream, a, b0, b1);
    const long long lanes = std::min<long long>((long long)n * h->spb, h->seg_cap);
    ORBFE_LAUNCH("k_gm_scatter", k_gm_scatter, dim3((unsigned)((lanes + GM_THREADS - 1) / GM_THREADS)), block, 0,
                 h->stream, a);
  }
  ORBFE_HIP_CHECK(hipGetLastError());
  ORBFE_HIP_CHECK(hipStreamSynchronize(h->stream));
  return ORBFE_OK;
}

static int gm_read_stats(orbfe_gridmap* h) {
  ORBFE_HIP_CHECK(hipMemcpyAsync(h->h_stat, h->d_stat, 8 * GM_ST_N, hipMemcpyDeviceToHost, h->stream));
  ORBFE_HIP_CHECK(hipStreamSynchronize(h->stream));
  return ORBFE_OK;
}

// the tallies of a finished update into the handle's dirty range and the caller's record
static void gm_finish_stats(orbfe_gridmap* h, orbfe_gridmap_stats* stats) {
  const long long* s = h->h_stat;
  if (s[GM_ST_ROW_MAX] >= 0) {
    const int r0 = (int)std::max<long long>(0, s[GM_ST_ROW_MIN]);
    const int r1 = (int)std::min<long long>(h->g.rows, s[GM_ST_ROW_MAX] + 1);
    if (h->dirty0 == h->dirty1) {
      h->dirty0 = r0;
      h->dirty1 = r1;
    } else {
      h->dirty0 = std::min(h->dirty0, r0);
      h->dirty1 = std::max(h->dirty1, r1);
    }
  }
  if (!stats) return;
  stats->beams = s[GM_ST_BEAMS];
  stats->visits = s[GM_ST_VISITS];
  stats->dropped = s[GM_ST_DROPPED];
  stats->points_cut = s[GM_ST_CUT];
  stats->kf_outside = (int32_t)s[GM_ST_KF_OUT];
  stats->row0 = h->dirty0;
  stats->row1 = h->dirty1;
}

// Keyframes k0 .. *k1 - 1: as many whole keyframes as GM_GROUP points hold; their regions in the handle's
// vectors. len[k]: the points (or slots) of keyframe k.
static int gm_next_group(orbfe_gridmap* h, int n_kf, int k0, const int32_t* len, int* k1) {
  h->kf_begin.clear();
  h->kf_len.clear();
  int k = k0, pts = 0;
  while (k < n_kf && pts + len[k] <= GM_GROUP) {
    h->kf_begin.push_back(pts);
    h->kf_len.push_back(len[k]);
    pts += len[k];
    k++;
  }
  *k1 = k;
  return pts;
}

static int gm_upload_group(orbfe_gridmap* h, const float* centres, int k0, int nk, bool with_count) {
  int32_t* d_begin = h->d_kf;
  int32_t* d_len = h->d_kf + ORBFE_GRIDMAP_MAX_KEYFRAMES;
  int32_t* d_count = h->d_kf + 2 * ORBFE_GRIDMAP_MAX_KEYFRAMES;
  ORBFE_HIP_CHECK(hipMemcpyAsync(h->d_centres, centres + 3 * (size_t)k0, 12 * (size_t)nk, hipMemcpyHostToDevice, h->stream));
  ORBFE_HIP_CHECK(hipMemcpyAsync(d_begin, h->kf_begin.data(), 4 * (size_t)nk, hipMemcpyHostToDevice, h->stream));
  ORBFE_HIP_CHECK(hipMemcpyAsync(d_len, h->kf_len.data(), 4 * (size_t)nk, hipMemcpyHostToDevice, h->stream));
  if (with_count)
    ORBFE_HIP_CHECK(hipMemcpyAsync(d_count, h->kf_len.data(), 4 * (size_t)nk, hipMemcpyHostToDevice, h->stream));
  return ORBFE_OK;
}

extern "C" int orbfe_gridmap_update(orbfe_gridmap* h, int n_kf, const float* centres, const int32_t* begin,
                                    const float* world_pos, orbfe_gridmap_stats* stats) {
  if (!h) return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_gridmap_update: bad argument");
  int st = gm_check_update(n_kf, centres, begin, world_pos);
  if (st) return orbfe_set_error(st, "orbfe_gridmap_update: bad keyframe list");
  if (h->device < 0) return orbfe_set_error(ORBFE_ERR_STATE, kGmHostOnly);
  hipSetDevice(h->device);
  std::vector<int32_t>& len = h->row_len;
  len.resize(n_kf);
  for (int k = 0; k < n_kf; k++) len[k] = begin[k + 1] - begin[k];
  ORBFE_LAUNCH("k_gm_stat_init", k_gm_stat_init, dim3(1), dim3(64), 0, h->stream, h->d_stat);
  for (int k0 = 0; k0 < n_kf;) {
    int k1 = k0;
    const int pts = gm_next_group(h, n_kf, k0, len.data(), &k1);
    st = gm_upload_group(h, centres, k0, k1 - k0, true);
    if (st) return st;
    if (pts > 0)
      ORBFE_HIP_CHECK(hipMemcpyAsync(h->d_pos, world_pos + 3 * (size_t)begin[k0], 12 * (size_t)pts, hipMemcpyHostToDevice,
                                     h->stream));
    GmArgs a = gm_args(h);
    a.n_kf = k1 - k0;
    a.n_pts = pts;
    st = gm_run_group(h, a, nullptr);
    if (st) return st;
    k0 = k1;
  }
  st = gm_read_stats(h);
  if (st) return st;
  gm_finish_stats(h, stats);
  return ORBFE_OK;
}

extern "C" int orbfe_gridmap_update_resident(orbfe_gridmap* h, orbfe_covis* covis, int n_kf, const int64_t* kf_ids,
                                             const float* centres, orbfe_gridmap_stats* stats, int32_t* n_missing) {
  if (!h || !covis || !centres) return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_gridmap_update_resident: bad argument");
  if (n_missing) *n_missing = 0;
  CovisRowsView v;
  int st = orbfe_covis_rows_view(covis, n_kf, kf_ids, &h->list_rows, &h->row_len, &v);
  if (st) return st;
  for (int k = 0; k < n_kf; k++)
    if (h->row_len[k] > ORBFE_GRIDMAP_MAX_POINTS)
      return orbfe_set_error(ORBFE_ERR_CAPACITY, "orbfe_gridmap_update_resident: a row of more than 8192 slots");
  if (h->device < 0) return orbfe_set_error(ORBFE_ERR_STATE, kGmHostOnly);
  if (v.device != h->device)
    return orbfe_set_error(ORBFE_ERR_STATE, "orbfe_gridmap_update_resident: the covisibility table is on another device");
  hipSetDevice(h->device);
  int32_t* d_list = h->d_kf + 3 * ORBFE_GRIDMAP_MAX_KEYFRAMES;
  GmRows r;
  r.rows = v.rows;
  r.row_n = v.row_n;
  r.bad = v.bad;
  r.rec = v.geo_rec;
  r.state = v.geo_rec ? v.geo_state : nullptr;
  r.M = v.M;
  r.S = v.S;
  r.P = v.P;
  r.list_rows = d_list;
  ORBFE_LAUNCH("k_gm_stat_init", k_gm_stat_init, dim3(1), dim3(64), 0, h->stream, h->d_stat);
  ORBFE_HIP_CHECK(hipMemcpyAsync(d_list, h->list_rows.data(), 4 * (size_t)n_kf, hipMemcpyHostToDevice, h->stream));
  const int max_row = *std::max_element(h->row_len.begin(), h->row_len.end());
  if (max_row > 0) {
    ORBFE_LAUNCH("k_gm_missing", k_gm_missing, dim3((max_row + GM_THREADS - 1) / GM_THREADS, n_kf), dim3(GM_THREADS), 0,
                 h->stream, r, h->d_stat);
    ORBFE_HIP_CHECK(hipGetLastError());
  }
  st = gm_read_stats(h);
  if (st) return st;
  if (h->h_stat[GM_ST_MISSING] > 0) {
    if (n_missing) *n_missing = (int32_t)h->h_stat[GM_ST_MISSING];
    return orbfe_set_error(ORBFE_ERR_STATE, "orbfe_gridmap_update_resident: a point's geometry was never set");
  }
  for (int k0 = 0; k0 < n_kf;) {
    int k1 = k0;
    const int pts = gm_next_group(h, n_kf, k0, h->row_len.data(), &k1);
    st = gm_upload_group(h, centres, k0, k1 - k0, false);
    if (st) return st;
    GmArgs a = gm_args(h);
    a.n_kf = k1 - k0;
    a.n_pts = pts;
    r.list_rows = d_list + k0;
    st = gm_run_group(h, a, &r);
    if (st) return st;
    k0 = k1;
  }
  st = gm_read_stats(h);
  if (st) return st;
  gm_finish_stats(h, stats);
  return ORBFE_OK;
}

extern "C" int orbfe_gridmap_build(orbfe_gridmap* h, int all_rows) {
  if (!h) return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_gridmap_build: bad argument");
  if (h->device < 0) return orbfe_set_error(ORBFE_ERR_STATE, kGmHostOnly);
  hipSetDevice(h->device);
  const int r0 = all_rows ? 0 : h->dirty0, r1 = all_rows ? h->g.rows : h->dirty1;
  if (r1 > r0) {
    const long long d0 = (long long)r0 * h->g.cols / 4, d1 = ((long long)r1 * h->g.cols + 3) / 4;
    ORBFE_LAUNCH("k_gm_build", k_gm_build, dim3((unsigned)((d1 - d0 + GM_THREADS - 1) / GM_THREADS)), dim3(GM_THREADS), 0,
                 h->stream, reinterpret_cast<const int4*>(h->d_occupied), reinterpret_cast<const int4*>(h->d_visits),
                 reinterpret_cast<uint32_t*>(h->d_grid), d0, std::min(d1, h->cells_pad / 4), h->g.visit_threshold);
    ORBFE_HIP_CHECK(hipGetLastError());
    ORBFE_HIP_CHECK(hipStreamSynchronize(h->stream));
  }
  h->dirty0 = h->dirty1 = 0;
  return ORBFE_OK;
}

static int gm_check_rows(const orbfe_gridmap* h, int row0, int row1, const char* what) {
  if (!h || row0 < 0 || row1 < row0 || row1 > h->g.rows) return orbfe_set_error(ORBFE_ERR_ARG, what);
  if (h->device < 0) return orbfe_set_error(ORBFE_ERR_STATE, kGmHostOnly);
  return ORBFE_OK;
}

extern "C" int orbfe_gridmap_download(orbfe_gridmap* h, int row0, int row1, int8_t* grid) {
  const int st = gm_check_rows(h, row0, row1, "orbfe_gridmap_download: bad argument");
  if (st) return st;
  if (row1 == row0) return ORBFE_OK;
  if (!grid) return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_gridmap_download: bad argument");
  hipSetDevice(h->device);
  const size_t lo = (size_t)row0 * h->g.cols, n = (size_t)(row1 - row0) * h->g.cols;
  ORBFE_HIP_CHECK(hipMemcpyAsync(grid, h->d_grid + lo, n, hipMemcpyDeviceToHost, h->stream));
  ORBFE_HIP_CHECK(hipStreamSynchronize(h->stream));
  return ORBFE_OK;
}

extern "C" int orbfe_gridmap_download_counters(orbfe_gridmap* h, int row0, int row1, int32_t* occupied,
                                               int32_t* visits) {
  const int st = gm_check_rows(h, row0, row1, "orbfe_gridmap_download_counters: bad argument");
  if (st) return st;
  if (row1 == row0) return ORBFE_OK;
  hipSetDevice(h->device);
  const size_t lo = (size_t)row0 * h->g.cols, n = (size_t)(row1 - row0) * h->g.cols;
  if (occupied) ORBFE_HIP_CHECK(hipMemcpyAsync(occupied, h->d_occupied + lo, 4 * n, hipMemcpyDeviceToHost, h->stream));
  if (visits) ORBFE_HIP_CHECK(hipMemcpyAsync(visits, h->d_visits + lo, 4 * n, hipMemcpyDeviceToHost, h->stream));
  ORBFE_HIP_CHECK(hipStreamSynchronize(h->stream));
  return ORBFE_OK;
}

extern "C" int orbfe_gridmap_upload_counters(orbfe_gridmap* h, int row0, int row1, const int32_t* occupied,
                                             const int32_t* visits) {
  const int st = gm_check_rows(h, row0, row1, "orbfe_gridmap_upload_counters: bad argument");
  if (st) return st;
  if (row1 == row0) return ORBFE_OK;
  hipSetDevice(h->device);
  const size_t lo = (size_t)row0 * h->g.cols, n = (size_t)(row1 - row0) * h->g.cols;
  if (occupied) ORBFE_HIP_CHECK(hipMemcpyAsync(h->d_occupied + lo, occupied, 4 * n, hipMemcpyHostToDevice, h->stream));
  if (visits) ORBFE_HIP_CHECK(hipMemcpyAsync(h->d_visits + lo, visits, 4 * n, hipMemcpyHostToDevice, h->stream));
  ORBFE_HIP_CHECK(hipStreamSynchronize(h->stream));
  if (h->dirty0 == h->dirty1) {
    h->dirty0 = row0;
    h->dirty1 = row1;
  } else {
    h->dirty0 = std::min(h->dirty0, row0);
    h->dirty1 = std::max(h->dirty1, row1);
  }
  return ORBFE_OK;
}

extern "C" int orbfe_gridmap_probability(orbfe_gridmap* h, int row0, int row1, float* data) {
  const int st = gm_check_rows(h, row0, row1, "orbfe_gridmap_probability: bad argument");
  if (st) return st;
  if (row1 == row0) return ORBFE_OK;
  if (!data) return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_gridmap_probability: bad argument");
  hipSetDevice(h->device);
  const long long lo = (long long)row0 * h->g.cols, hi = (long long)row1 * h->g.cols;
  for (long long c = lo; c < hi; c += GM_PROB_CHUNK) {
    const int n = (int)std::min<long long>(GM_PROB_CHUNK, hi - c);
    ORBFE_LAUNCH("k_gm_probability", k_gm_probability, dim3((n + GM_THREADS - 1) / GM_THREADS), dim3(GM_THREADS), 0,
                 h->stream, (const int32_t*)h->d_occupied, (const int32_t*)h->d_visits, c, n, h->g.visit_threshold,
                 h->d_prob);
    ORBFE_HIP_CHECK(hipGetLastError());
    ORBFE_HIP_CHECK(hipMemcpyAsync(data + (c - lo), h->d_prob, 4 * (size_t)n, hipMemcpyDeviceToHost, h->stream));
    ORBFE_HIP_CHECK(hipStreamSynchronize(h->stream));
  }
  return ORBFE_OK;
}
