// orbfe_covis.hip -- the covisibility table on gfx950: the keyframes' mvpMapPoints rows resident on
// the device, the observations derived from them, and the three walks of the reference over them.
//
// Reference: src/KeyFrame.cc:304-378 (UpdateConnections), src/Tracking.cc:1257-1303
// (UpdateLocalKeyFrames' vote), src/Optimizer.cc:471-506 (LocalBundleAdjustment's gather).
// include/orbfe_covis.h lists the semantics; orbfe_covis_core.h holds the host bookkeeping.
//
// Device layout: rows[M * S] (point id per slot, -1: none), row_n[M] (-1: free row), bad[P], and
// three int32 arrays of P + 1 entries (a: the inverse's CSR begin; b, c: scratch of the rebuild and
// of the local-map gather). Every per-point pass runs over n_pts = 1 + the largest id ever written.
// An inverse entry is one uint32: bit 31 "the keyframe already appears with a lower slot", bits
// 13-24 the keyframe's rank by mnId, bits 0-12 the slot; a segment is ascending in that word.
// The host uploads two rank tables whenever the keyframe set changes: mnId rank per row, and tie
// rank per mnId rank. The vote's histogram is indexed by tie rank, so its non-zero bins in index
// order are the reference's std::map iteration, and weight << 12 | tie rank is the sort key.
//
// Rebuild (after any row mutation): k_covis_count (atomic count per point) -> exclusive scan
// (k_covis_scan_local / _tops / _add, 4096 entries per workgroup, at most 4096 workgroups) ->
// k_covis_fill (atomic cursor per point; order within a segment arbitrary) -> k_covis_canon (each
// entry finds its place by counting the smaller words of its segment, and learns whether it is a
// repeat of its keyframe).
// k_covis_vote: one 1024-thread workgroup per query; a 4096-bin uint32 histogram (16 KiB) and 4096
// sort keys (16 KiB) in LDS. Threads stride over the query's slots, walk each point's observers and
// add with LDS atomics (integer, order-free). The bins are compacted with one block scan (counter),
// the bins >= th go to the key array and are bitonic-sorted descending, 1024 keys per pass.
// Local map: k_covis_lm_mark (points of the local rows) -> k_covis_lm_count (edges per marked
// point) -> two scans -> k_covis_lm_emit (points, CSR, raw edges, seen keyframes) ->
// k_covis_lm_order (one workgroup: local then fixed, both ascending in mnId rank) -> k_covis_lm_edges.
// The ordered distinct union of rows and the geometry store (include/orbfe_localmap.h) are at the end of
// the file: k_lm_first -> k_lm_count -> scan -> k_lm_emit -> (k_lm_gather, k_lm_seen) -> k_lm_reset.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/orbfe.h"
#include "../../include/orbfe_covis.h"
#include "../../include/orbfe_localmap.h"
#include "orbfe_covis_core.h"
#include "orbfe_covis_view.h"
#include "orbfe_cull_core.h"
#include "orbfe_device.h"
#include "orbfe_ktimer.h"
#include "orbfe_localmap_core.h"
#include "orbfe_stage.h"

namespace cc = orbfe_covis_core;
namespace lm = orbfe_localmap_core;

#define COVIS_THREADS 1024
#define COVIS_BINS 4096       // = ORBFE_COVIS_MAX_KEYFRAMES = 4 per thread
#define COVIS_SCAN_TILE 4096  // entries per workgroup of the scan
#define COVIS_ROW_THREADS 256

static_assert(COVIS_BINS == ORBFE_COVIS_MAX_KEYFRAMES && COVIS_BINS == 4 * COVIS_THREADS, "4 bins per thread");
static_assert(ORBFE_COVIS_MAX_SLOTS == 1 << 13, "13 slot bits in an inverse entry");
static_assert(ORBFE_COVIS_MAX_POINT_ID <= COVIS_SCAN_TILE * 4096, "the scan's second level is one workgroup");

// Exclusive scan of 4 values per thread over a 1024-thread workgroup, thread-major; returns the
// total. s_wsum: 16 ints of LDS. Contains __syncthreads(): uniform control flow only.
__device__ __forceinline__ int covis_block_scan4(int (&v)[4], int* s_wsum) {
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
  for (int k = 0; k < COVIS_THREADS / 64; k++) {
    const int x = s_wsum[k];
    off += k < w ? x : 0;
    total += x;
  }
  __syncthreads();  // s_wsum may be written again
  int run = off + inc - s;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int x = v[j];
    v[j] = run;
    run += x;
  }
  return total;
}

// data[0..n) -> exclusive scan within each 4096-entry tile, the tile's total to tops[tile]
__global__ __launch_bounds__(COVIS_THREADS) void k_covis_scan_local(int32_t* data, int n, int32_t* tops) {
  __shared__ int s_wsum[COVIS_THREADS / 64];
  const long long base = (long long)blockIdx.x * COVIS_SCAN_TILE + (int)threadIdx.x * 4;
  int v[4];
#pragma unroll
  for (int j = 0; j < 4; j++) v[j] = base + j < n ? data[base + j] : 0;
  const int total = covis_block_scan4(v, s_wsum);
#pragma unroll
  for (int j = 0; j < 4; j++)
    if (base + j < n) data[base + j] = v[j];
  if (threadIdx.x == 0) tops[blockIdx.x] = total;
}

// tops[0..nb) (nb <= 4096) -> exclusive scan, the grand total to *total_out
__global__ __launch_bounds__(COVIS_THREADS) void k_covis_scan_tops(int32_t* tops, int nb, int32_t* total_out) {
  __shared__ int s_wsum[COVIS_THREADS / 64];
  const int base = (int)threadIdx.x * 4;
  int v[4];
#pragma unroll
  for (int j = 0; j < 4; j++) v[j] = base + j < nb ? tops[base + j] : 0;
  const int total = covis_block_scan4(v, s_wsum);
#pragma unroll
  for (int j = 0; j < 4; j++)
    if (base + j < nb) tops[base + j] = v[j];
  if (threadIdx.x == 0) *total_out = total;
}

__global__ __launch_bounds__(COVIS_THREADS) void k_covis_scan_add(int32_t* data, int n, const int32_t* tops) {
  const int add = tops[blockIdx.x];
  const long long base = (long long)blockIdx.x * COVIS_SCAN_TILE + (int)threadIdx.x * 4;
#pragma unroll
  for (int j = 0; j < 4; j++)
    if (base + j < n) data[base + j] += add;
}

struct CovisTable {
  int32_t* rows;    // [M * S]
  int32_t* row_n;   // [M]
  uint8_t* bad;     // [P]
  int32_t* begin;   // [P + 1] the inverse's CSR (a)
  uint32_t* obs;    // [obs_cap] the inverse's entries
  int S;
  int n_pts;        // per-point arrays are valid over 0..n_pts
  int n_live;
};

// grid (ceil(max row / 256), rows ever used): one thread per slot
__global__ __launch_bounds__(COVIS_ROW_THREADS) void k_covis_count(CovisTable t, int32_t* cnt) {
  const int k = blockIdx.y, s = (int)(blockIdx.x * COVIS_ROW_THREADS + threadIdx.x);
  if (s >= t.row_n[k] || s >= t.S) return;
  const int p = t.rows[(size_t)k * t.S + s];
  if ((unsigned)p < (unsigned)t.n_pts) atomicAdd(&cnt[p], 1);
}

__global__ __launch_bounds__(COVIS_ROW_THREADS) void k_covis_fill(CovisTable t, int32_t* cursor,
                                                                  const int32_t* id_rank_of_row,
                                                                  unsigned long long* tmp, long long cap) {
  const int k = blockIdx.y, s = (int)(blockIdx.x * COVIS_ROW_THREADS + threadIdx.x);
  if (s >= t.row_n[k] || s >= t.S) return;
  const int p = t.rows[(size_t)k * t.S + s];
  if ((unsigned)p >= (unsigned)t.n_pts) return;
  const long long e = (long long)t.begin[p] + atomicAdd(&cursor[p], 1);
  if (e < cap) tmp[e] = ((unsigned long long)p << 32) | (uint32_t)((id_rank_of_row[k] << 13) | s);
}

// One thread per entry: its place in the segment is the number of smaller words there (the words
// of a segment are distinct); it is a repeat when a smaller word names the same keyframe.
__global__ __launch_bounds__(COVIS_ROW_THREADS) void k_covis_canon(CovisTable t, const unsigned long long* tmp,
                                                                   long long cap) {
  const long long e = (long long)blockIdx.x * COVIS_ROW_THREADS + threadIdx.x;
  if (e >= cap || e >= t.begin[t.n_pts]) return;
  const unsigned long long x = tmp[e];
  const int p = (int)(x >> 32);
  const uint32_t key = (uint32_t)x;
  if ((unsigned)p >= (unsigned)t.n_pts) return;
  const int b = t.begin[p], n = t.begin[p + 1] - b;
  int rank = 0;
  uint32_t dup = 0;
  for (int j = 0; j < n; j++) {
    const uint32_t kj = (uint32_t)tmp[b + j];
    if (kj < key) {
      rank++;
      if ((kj >> 13) == (key >> 13)) dup = 1u << 31;
    }
  }
  t.obs[b + rank] = key | dup;
}

// grid ceil(n / 256): rows[row * S + slots[i]] = ids[i] (the host has made the slots distinct)
__global__ __launch_bounds__(COVIS_ROW_THREADS) void k_covis_scatter(int32_t* row, int row_len, int n,
                                                                     const int32_t* slots, const int32_t* ids) {
  const int i = (int)(blockIdx.x * COVIS_ROW_THREADS + threadIdx.x);
  if (i < n && (unsigned)slots[i] < (unsigned)row_len) row[slots[i]] = ids[i];
}

__global__ __launch_bounds__(COVIS_ROW_THREADS) void k_covis_set_bad(uint8_t* bad, int P, int n, const int32_t* ids,
                                                                     int flag) {
  const int i = (int)(blockIdx.x * COVIS_ROW_THREADS + threadIdx.x);
  if (i < n && (unsigned)ids[i] < (unsigned)P) bad[ids[i]] = (uint8_t)flag;
}

struct CovisVoteArgs {
  CovisTable t;
  const uint16_t* tie_of_idrank;  // [n_live]
  const int32_t* q_row;           // [n] row per query; NULL: the queries are point lists
  const int32_t* q_self;          // [n] the query's own tie rank (excluded)
  const int32_t* q_begin;         // [n + 1] CSR of point lists
  const int32_t* q_points;
  int th, want_ordered;
  int stride;                     // entries per list in out
  uint32_t* out;                  // per query: {n_counter, n_ordered, nmax, rank of kf_max}, counter[stride], ordered[stride]
};

__global__ __launch_bounds__(COVIS_THREADS) void k_covis_vote(CovisVoteArgs a) {
  __shared__ uint32_t s_hist[COVIS_BINS];
  __shared__ uint32_t s_keys[COVIS_BINS];
  __shared__ int s_wsum[COVIS_THREADS / 64];
  __shared__ int s_best;
  const int tid = threadIdx.x, q = blockIdx.x;
  for (int i = tid; i < COVIS_BINS; i += COVIS_THREADS) s_hist[i] = 0;
  if (tid == 0) s_best = 0;
  __syncthreads();
  const int32_t* src;
  int len, self;
  if (a.q_row) {
    const int k = a.q_row[q];
    len = min(max(a.t.row_n[k], 0), a.t.S);
    src = a.t.rows + (size_t)k * a.t.S;
    self = a.q_self[q];
  } else {
    const int b = a.q_begin[q];
    len = min(max(a.q_begin[q + 1] - b, 0), ORBFE_COVIS_MAX_SLOTS);
    src = a.q_points + b;
    self = -1;
  }
  for (int i = tid; i < len; i += COVIS_THREADS) {
    const int p = src[i];
    if ((unsigned)p >= (unsigned)a.t.n_pts) continue;  // -1: no point
    if (a.t.bad[p]) continue;                           // isBad()
    const int e1 = a.t.begin[p + 1];
    for (int e = a.t.begin[p]; e < e1; e++) {
      const uint32_t v = a.t.obs[e];
      if (v >> 31) continue;  // the keyframe was counted at its lowest slot
      const int r = a.tie_of_idrank[(v >> 13) & 4095u];
      if (r != self && r < a.t.n_live) atomicAdd(&s_hist[r], 1u);
    }
  }
  __syncthreads();
  // bins 4 * tid .. + 3: counter entries in the low half of the scan word, entries >= th in the high
  uint32_t w[4];
  int v[4];
  int lbest = 0;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int r = tid * 4 + j;
    w[j] = s_hist[r];
    const bool ge = a.want_ordered && w[j] > 0 && (long long)w[j] >= (long long)a.th;
    v[j] = (w[j] > 0 ? 1 : 0) | (ge ? 1 << 16 : 0);
    // the maximum, and among equals the lowest tie rank (the strict > while iterating ascending)
    if (w[j] > 0) lbest = max(lbest, (int)((w[j] << 12) | (uint32_t)(COVIS_BINS - 1 - r)));
  }
  const int total = covis_block_scan4(v, s_wsum);
  const int n_counter = total & 0xffff, n_ord = total >> 16;
  uint32_t* out = a.out + (size_t)q * (4 + 2 * (size_t)a.stride);
#pragma unroll
  for (int j = 0; j < 4; j++) {
    if (w[j] == 0) continue;
    const uint32_t key = (w[j] << 12) | (uint32_t)(tid * 4 + j);
    const int pos = v[j] & 0xffff;
    if (pos < a.stride) out[4 + pos] = key;
    if (a.want_ordered && (long long)w[j] >= (long long)a.th) s_keys[v[j] >> 16] = key;
  }
  lbest = wave_max(lbest);
  if (lane_id() == 0) atomicMax(&s_best, lbest);
  int P2 = 64;
  while (P2 < n_ord) P2 <<= 1;
  __syncthreads();
  for (int i = n_ord + tid; i < P2; i += COVIS_THREADS) s_keys[i] = 0;  // below every key (weight >= 1)
  __syncthreads();
  if (n_ord > 1) {  // block-uniform
    for (int k = 2; k <= P2; k <<= 1) {
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int i = tid; i < P2; i += COVIS_THREADS) {
          const int x = i ^ j;
          if (x > i) {
            const uint32_t u = s_keys[i], z = s_keys[x];
            if ((u < z) == ((i & k) == 0)) {  // descending
              s_keys[i] = z;
              s_keys[x] = u;
            }
          }
        }
        __syncthreads();
      }
    }
  }
  for (int i = tid; i < n_ord && i < a.stride; i += COVIS_THREADS) out[4 + a.stride + i] = s_keys[i];
  if (tid == 0) {
    const uint32_t best = (uint32_t)s_best;
    const uint32_t nmax = best >> 12, rmax = (uint32_t)(COVIS_BINS - 1) - (best & 4095u);
    int n_ordered = n_ord;
    if (a.want_ordered && n_ord == 0 && n_counter > 0) {  // KeyFrame.cc:364-368
      n_ordered = 1;
      if (a.stride > 0) out[4 + a.stride] = (nmax << 12) | rmax;
    }
    out[0] = (uint32_t)n_counter;
    out[1] = (uint32_t)n_ordered;
    out[2] = nmax;
    out[3] = n_counter > 0 ? rmax : 0xffffffffu;
  }
}

// grid (ceil(max row / 256), n_local): mark[p] = 1 for the non-bad points of the local rows
__global__ __launch_bounds__(COVIS_ROW_THREADS) void k_covis_lm_mark(CovisTable t, const int32_t* local_rows,
                                                                     int32_t* mark) {
  const int k = local_rows[blockIdx.y], s = (int)(blockIdx.x * COVIS_ROW_THREADS + threadIdx.x);
  if (s >= t.row_n[k] || s >= t.S) return;
  const int p = t.rows[(size_t)k * t.S + s];
  if ((unsigned)p < (unsigned)t.n_pts && !t.bad[p]) mark[p] = 1;
}

// ecnt[p] = observers of a marked point, else 0
__global__ __launch_bounds__(COVIS_ROW_THREADS) void k_covis_lm_count(CovisTable t, const int32_t* mark,
                                                                      int32_t* ecnt) {
  const int p = (int)(blockIdx.x * COVIS_ROW_THREADS + threadIdx.x);
  if (p >= t.n_pts) return;
  int c = 0;
  if (mark[p]) {
    const int e1 = t.begin[p + 1];
    for (int e = t.begin[p]; e < e1; e++) c += (t.obs[e] >> 31) ? 0 : 1;
  }
  ecnt[p] = c;
}

struct CovisEmitArgs {
  CovisTable t;
  const int32_t* pidx;   // [n_pts + 1] scanned marks
  const int32_t* ebeg;   // [n_pts + 1] scanned edge counts
  int pt_cap, edge_cap;
  int32_t* hdr;          // {n_points, n_edges, n_fixed, 0}
  int32_t* out_points;   // [pt_cap]
  int32_t* out_ebeg;     // [pt_cap + 1]
  int32_t* edge_kf;      // [edge_cap] the observer's mnId rank; k_covis_lm_edges maps it
  int32_t* edge_slot;    // [edge_cap]
  int32_t* seen;         // [n_live] by mnId rank
};

__global__ __launch_bounds__(COVIS_ROW_THREADS) void k_covis_lm_emit(CovisEmitArgs a) {
  const int p = (int)(blockIdx.x * COVIS_ROW_THREADS + threadIdx.x);
  if (p >= a.t.n_pts) return;
  if (p == 0) {
    const int np = a.pidx[a.t.n_pts], ne = a.ebeg[a.t.n_pts];
    a.hdr[0] = np;
    a.hdr[1] = ne;
    if (np <= a.pt_cap) a.out_ebeg[np] = ne;
  }
  const int i = a.pidx[p];
  if (a.pidx[p + 1] == i) return;  // not marked
  int e = a.ebeg[p];
  if (i < a.pt_cap) {
    a.out_points[i] = p;
    a.out_ebeg[i] = e;
  }
  const int o1 = a.t.begin[p + 1];
  for (int o = a.t.begin[p]; o < o1; o++) {
    const uint32_t v = a.t.obs[o];
    if (v >> 31) continue;
    const int r = (int)((v >> 13) & 4095u);
    if (r < a.t.n_live) a.seen[r] = 1;
    if (e < a.edge_cap) {
      a.edge_kf[e] = r;
      a.edge_slot[e] = (int)(v & 8191u);
    }
    e++;
  }
}

// One workgroup over the mnId ranks: local keyframes first, then the seen ones that are not local.
__global__ __launch_bounds__(COVIS_THREADS) void k_covis_lm_order(int n_live, int n_local, const uint8_t* is_local,
                                                                  const int32_t* seen, int32_t* order, int fixed_cap,
                                                                  int32_t* out_fixed, int32_t* hdr) {
  __shared__ int s_wsum[COVIS_THREADS / 64];
  const int tid = threadIdx.x;
  int v[4], kind[4];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int r = tid * 4 + j;
    kind[j] = 0;
    if (r < n_live) kind[j] = is_local[r] ? 1 : (seen[r] ? 2 : 0);
    v[j] = kind[j] == 1 ? 1 : (kind[j] == 2 ? 1 << 16 : 0);
  }
  const int total = covis_block_scan4(v, s_wsum);
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int r = tid * 4 + j;
    if (kind[j] == 1) {
      order[r] = v[j] & 0xffff;
    } else if (kind[j] == 2) {
      const int f = v[j] >> 16;
      order[r] = n_local + f;
      if (f < fixed_cap) out_fixed[f] = r;
    }
  }
  if (tid == 0) hdr[2] = total >> 16;
}

__global__ __launch_bounds__(COVIS_ROW_THREADS) void k_covis_lm_edges(const int32_t* hdr, int edge_cap, int n_live,
                                                                      const int32_t* order, int32_t* edge_kf) {
  const int e = (int)(blockIdx.x * COVIS_ROW_THREADS + threadIdx.x);
  if (e >= edge_cap || e >= hdr[1]) return;
  const int r = edge_kf[e];
  if ((unsigned)r < (unsigned)n_live) edge_kf[e] = order[r];
}

// ---- culling (orbfe_cull_core.h holds the per-item rules) -----------------------------------
// The inverse is the one the call started with; what the call itself changes is read beside it: the
// rows (a bad point's recorded slots become -1), the bad flags, and `culled`, indexed by mnId rank.
// k_covis_cull_eval: one 256-thread workgroup per undecided candidate, threads stride over the slots.
// k_covis_cull_commit: one 1024-thread workgroup applies the round's lowest culling candidate.
// k_covis_cull_points: one thread per recent point.
#define COVIS_CULL_NONE 0x7f7f7f7f  // a round's minimum before any candidate culls (memset bytes 0x7f)

struct CovisCullArgs {
  CovisTable t;
  int M;
  const uint8_t* attr;            // [M * S]
  const int32_t* row_at_idrank;   // [n_live]
  const int32_t* id_rank_of_row;  // [M]
  int32_t* culled;                // [n_live] by mnId rank
  const int32_t* cand_row;        // [n]
  const uint8_t* cand_flag;       // [n] bit 0: not_erase, bit 1: mnId 0
  int n, start, monocular;
  uint8_t* decision;              // [n]
  int32_t* n_mps;                 // [n]
  int32_t* n_red;                 // [n]
  int32_t* round_min;             // this round's lowest index that culls
  int32_t* bad_count;             // [n]
  int32_t* bad_list;              // [bad_cap]
  int32_t* bad_cursor;            // entries of bad_list in use
  int bad_cap;
};

// Observations() of p and the gated observers other than `self`, over the live observers that this
// call has not culled. attr_slot: the candidate's byte at the querying slot.
__device__ __forceinline__ void covis_cull_walk(const CovisCullArgs& a, int p, int self, uint8_t attr_slot,
                                                int* obs_out, int* gated_out, int* self_slot_out) {
  int obs = 0, gated = 0, self_slot = -1;
  const int e1 = a.t.begin[p + 1];
  for (int e = a.t.begin[p]; e < e1; e++) {
    const uint32_t v = a.t.obs[e];
    if (v >> 31) continue;  // the keyframe is recorded at its lowest slot
    const int r = (int)((v >> 13) & 4095u);
    if (r >= a.t.n_live) continue;
    const int os = (int)(v & 8191u);
    if (r == self) self_slot = os;
    if (a.culled && a.culled[r]) continue;
    const int orow = a.row_at_idrank[r];
    if ((unsigned)orow >= (unsigned)a.M || os >= a.t.S) continue;
    const uint8_t ao = a.attr[(size_t)orow * a.t.S + os];
    obs += cull_weight(ao);
    if (r != self && cull_gate(ao, attr_slot)) gated++;
  }
  *obs_out = obs;
  *gated_out = gated;
  *self_slot_out = self_slot;
}

// SetBadFlag of p: the flag, and -1 at the recorded slot of every observer still alive
__device__ __forceinline__ void covis_cull_set_bad(const CovisCullArgs& a, int p, int self) {
  a.t.bad[p] = 1;
  if (p >= a.t.n_pts) return;
  const int e1 = a.t.begin[p + 1];
  for (int e = a.t.begin[p]; e < e1; e++) {
    const uint32_t v = a.t.obs[e];
    if (v >> 31) continue;
    const int r = (int)((v >> 13) & 4095u);
    if (r >= a.t.n_live || r == self) continue;
    if (a.culled && a.culled[r]) continue;
    const int orow = a.row_at_idrank[r], os = (int)(v & 8191u);
    if ((unsigned)orow >= (unsigned)a.M || os >= a.t.S || os >= a.t.row_n[orow]) continue;
    int32_t* cell = a.t.rows + (size_t)orow * a.t.S + os;
    if (*cell == p) *cell = -1;
  }
}

// grid n - start: candidate start + blockIdx.x
__global__ __launch_bounds__(COVIS_ROW_THREADS) void k_covis_cull_eval(CovisCullArgs a) {
  __shared__ int s_mps[COVIS_ROW_THREADS / 64], s_red[COVIS_ROW_THREADS / 64];
  const int c = a.start + (int)blockIdx.x, tid = threadIdx.x;
  if (c >= a.n) return;
  const int flag = a.cand_flag[c];
  if (flag & 2) {
    if (tid == 0) {
      a.decision[c] = CULL_SKIPPED;
      a.n_mps[c] = 0;
      a.n_red[c] = 0;
    }
    return;
  }
  const int row = a.cand_row[c];
  if ((unsigned)row >= (unsigned)a.M) return;
  const int len = min(max(a.t.row_n[row], 0), a.t.S);
  const int self = a.id_rank_of_row[row];
  const size_t base = (size_t)row * a.t.S;
  int mps = 0, red = 0;
  for (int i = tid; i < len; i += COVIS_ROW_THREADS) {
    const int p = a.t.rows[base + i];
    if ((unsigned)p >= (unsigned)a.t.n_pts) continue;
    const uint8_t at = a.attr[base + i];
    if (!cull_slot_counted(p, a.t.bad[p], at, a.monocular)) continue;
    mps++;
    int obs, gated, self_slot;
    covis_cull_walk(a, p, self, at, &obs, &gated, &self_slot);
    if (cull_slot_redundant(obs, gated)) red++;
  }
  mps = wave_sum(mps);
  red = wave_sum(red);
  if (lane_id() == 0) {
    s_mps[wave_id()] = mps;
    s_red[wave_id()] = red;
  }
  __syncthreads();
  if (tid == 0) {
    int m = 0, r = 0;
    for (int w = 0; w < COVIS_ROW_THREADS / 64; w++) {
      m += s_mps[w];
      r += s_red[w];
    }
    const int d = cull_decision(r, m, flag & 1);
    a.decision[c] = (uint8_t)d;
    a.n_mps[c] = m;
    a.n_red[c] = r;
    if (d == CULL_CULLED) atomicMin(a.round_min, c);
  }
}

// One workgroup. EraseObservation(this) on every first-occurrence slot of the culled row in slot order
// (the list order comes from the block scan), then the row leaves the table.
__global__ __launch_bounds__(COVIS_THREADS) void k_covis_cull_commit(CovisCullArgs a) {
  __shared__ int s_wsum[COVIS_THREADS / 64];
  const int c = *a.round_min, tid = threadIdx.x;
  if (c < 0 || c >= a.n) return;  // nobody culls: the call is decided
  const int row = a.cand_row[c];
  if ((unsigned)row >= (unsigned)a.M) return;
  const int len = min(max(a.t.row_n[row], 0), a.t.S);
  const int self = a.id_rank_of_row[row];
  const size_t base = (size_t)row * a.t.S;
  const int cursor = *a.bad_cursor;
  __syncthreads();  // row_n[row] and the cursor are rewritten below
  int run = 0;
  for (int chunk = 0; chunk < len; chunk += 4 * COVIS_THREADS) {
    int v[4], pt[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int i = chunk + tid * 4 + j;
      v[j] = 0;
      pt[j] = -1;
      if (i >= len) continue;
      const int p = a.t.rows[base + i];
      if ((unsigned)p >= (unsigned)a.t.n_pts) continue;
      if (a.t.bad[p]) continue;  // its observations are gone already
      int obs, gated, self_slot;
      covis_cull_walk(a, p, self, 0, &obs, &gated, &self_slot);
      if (self_slot != i) continue;  // held in a lower slot too: erased there
      const uint8_t own = a.attr[base + i];
      if (cull_point_goes_bad(obs - cull_weight(own))) {
        v[j] = 1;
        pt[j] = p;
      }
    }
    __syncthreads();  // every flag of the chunk was read before one is written
    const int total = covis_block_scan4(v, s_wsum);
#pragma unroll
    for (int j = 0; j < 4; j++) {
      if (pt[j] < 0) continue;
      const int at = cursor + run + v[j];
      if (at < a.bad_cap) a.bad_list[at] = pt[j];
      covis_cull_set_bad(a, pt[j], self);
    }
    run += total;
  }
  __syncthreads();
  if (tid == 0) {
    a.culled[self] = 1;
    a.t.row_n[row] = -1;
    a.bad_count[c] = run;
    *a.bad_cursor = cursor + run;
  }
}

struct CovisCullPointsArgs {
  CovisCullArgs a;  // the table part; culled = NULL
  int n_points;
  const int32_t* ids;
  const int32_t* found;
  const int32_t* visible;
  const long long* first;
  long long current;
  uint8_t* action;
  int P;
};

__global__ __launch_bounds__(COVIS_ROW_THREADS) void k_covis_cull_points(CovisCullPointsArgs q) {
  const int i = (int)(blockIdx.x * COVIS_ROW_THREADS + threadIdx.x);
  if (i >= q.n_points) return;
  const int p = q.ids[i];
  if ((unsigned)p >= (unsigned)q.P) return;
  int obs = 0, gated, self_slot;
  if (p < q.a.t.n_pts) covis_cull_walk(q.a, p, -1, 0, &obs, &gated, &self_slot);
  const int act = cull_point_action(q.a.t.bad[p], q.found[i], q.visible[i], q.current, q.first[i], obs, q.a.monocular);
  q.action[i] = (uint8_t)act;
  if (act == CULL_PT_RATIO || act == CULL_PT_OBS) covis_cull_set_bad(q.a, p, -1);
}

// ------------------------------------------------------------------------------------------
// host

struct orbfe_covis : OrbfeDev {
  cc::Core core;
  int32_t* d_rows = nullptr;
  int32_t* d_row_n = nullptr;
  uint8_t* d_bad = nullptr;
  int32_t* d_a = nullptr;  // [P + 1] inverse begin
  int32_t* d_b = nullptr;  // [P + 1]
  int32_t* d_c = nullptr;  // [P + 1]
  int32_t* d_tops = nullptr;             // [4096]
  int32_t* d_id_rank_of_row = nullptr;   // [M]
  uint16_t* d_tie_of_idrank = nullptr;   // [M]
  uint8_t* d_is_local = nullptr;         // [M]
  int32_t* d_seen = nullptr;             // [M]
  int32_t* d_order = nullptr;            // [M]
  uint8_t* d_attr = nullptr;             // [M * S] one attribute byte per row slot
  int32_t* d_row_at_idrank = nullptr;    // [M]
  int32_t* d_culled = nullptr;           // [M] by mnId rank: culled in this call
  unsigned long long* d_tmp = nullptr;   // [obs_cap]
  uint32_t* d_obs = nullptr;             // [obs_cap]
  long long obs_cap = 0;
  uint8_t* h_stage = nullptr;  // pinned uploads of one call
  uint8_t* d_stage = nullptr;
  size_t stage_cap = 0, stage_used = 0;
  uint8_t* h_res = nullptr;    // pinned result of one call
  uint8_t* d_res = nullptr;
  size_t res_cap = 0;
  std::vector<int32_t> tmp_rows, tmp_slots, tmp_ids;
  // include/orbfe_localmap.h, each allocated on first use
  uint32_t* d_lm_first = nullptr;  // [P] all ones between calls
  bool lm_dirty = false;           // a call was cut short: d_lm_first is refilled whole by the next one
  uint8_t* d_geo_rec = nullptr;    // [P * 64] the geometry store
  uint8_t* d_geo_state = nullptr;  // [P] stored flags | lm::kPresent
  uint8_t* d_geo_out = nullptr;    // the gathered SoA of one call: 65 bytes per point, geo_out_cap points
  int geo_out_cap = 0;
};

static int covis_fail(const char* fn, const cc::Status& st) {
  return orbfe_set_error(st.code, (std::string(fn) + ": " + st.msg).c_str());
}

// Room for one call's uploads (`bytes` counts each piece rounded up to 256).
static int covis_stage_reserve(orbfe_covis* h, size_t bytes) {
  h->stage_used = 0;
  if (bytes <= h->stage_cap) return ORBFE_OK;
  ORBFE_HIP_CHECK(hipStreamSynchronize(h->stream));
  if (h->h_stage) hipHostFree(h->h_stage);
  if (h->d_stage) hipFree(h->d_stage);
  h->h_stage = nullptr;
  h->d_stage = nullptr;
  h->stage_cap = 0;
  const size_t cap = orbfe_al256(bytes + bytes / 2);
  ORBFE_HIP_CHECK(hipHostMalloc((void**)&h->h_stage, cap, hipHostMallocDefault));
  ORBFE_HIP_CHECK(hipMalloc((void**)&h->d_stage, cap));
  h->stage_cap = cap;
  return ORBFE_OK;
}

static size_t covis_stage_take(orbfe_covis* h, size_t bytes) {
  const size_t off = h->stage_used;
  h->stage_used += orbfe_al256(bytes);
  return off;
}

// Copies `bytes` of src through the pinned staging to dst (NULL: the staging's own device side);
// returns the device address through *dev.
static int covis_upload(orbfe_covis* h, const void* src, size_t bytes, void* dst, const void** dev) {
  const size_t off = covis_stage_take(h, bytes);
  if (off + bytes > h->stage_cap) return orbfe_set_error(ORBFE_ERR_STATE, "orbfe_covis: staging overrun");
  void* d = dst ? dst : (void*)(h->d_stage + off);
  if (bytes > 0) {
    memcpy(h->h_stage + off, src, bytes);
    ORBFE_HIP_CHECK(hipMemcpyAsync(d, h->h_stage + off, bytes, hipMemcpyHostToDevice, h->stream));
  }
  if (dev) *dev = d;
  return ORBFE_OK;
}

static int covis_res_reserve(orbfe_covis* h, size_t bytes) {
  if (bytes <= h->res_cap) return ORBFE_OK;
  ORBFE_HIP_CHECK(hipStreamSynchronize(h->stream));
  if (h->h_res) hipHostFree(h->h_res);
  if (h->d_res) hipFree(h->d_res);
  h->h_res = nullptr;
  h->d_res = nullptr;
  h->res_cap = 0;
  const size_t cap = orbfe_al256(bytes + bytes / 2);
  ORBFE_HIP_CHECK(hipHostMalloc((void**)&h->h_res, cap, hipHostMallocDefault));
  ORBFE_HIP_CHECK(hipMalloc((void**)&h->d_res, cap));
  h->res_cap = cap;
  return ORBFE_OK;
}

extern "C" int orbfe_covis_create(int device, int max_keyframes, int max_slots, int max_point_id,
                                  orbfe_covis** out) {
  if (!out) return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_covis_create: bad argument");
  *out = nullptr;
  cc::Status cs = cc::Core::check_create(max_keyframes, max_slots, max_point_id);
  if (cs) return covis_fail("orbfe_covis_create", cs);
  orbfe_covis* h = new orbfe_covis();
  h->core.init(max_keyframes, max_slots, max_point_id);
  if (device < 0) {
    *out = h;
    return ORBFE_OK;
  }
  const int open_st = orbfe_dev_open(h, device, "orbfe_covis_create");
  if (open_st != ORBFE_OK) {
    orbfe_covis_destroy(h);
    return open_st;
  }
  const size_t M = (size_t)max_keyframes, S = (size_t)max_slots, P = (size_t)max_point_id;
  ORBFE_CREATE_HIP(h, orbfe_covis_destroy, hipMalloc((void**)&h->d_rows, 4 * M * S));
  ORBFE_CREATE_HIP(h, orbfe_covis_destroy, hipMalloc((void**)&h->d_row_n, 4 * M));
  ORBFE_CREATE_HIP(h, orbfe_covis_destroy, hipMalloc((void**)&h->d_bad, P));
  ORBFE_CREATE_HIP(h, orbfe_covis_destroy, hipMalloc((void**)&h->d_a, 4 * (P + 1)));
  ORBFE_CREATE_HIP(h, orbfe_covis_destroy, hipMalloc((void**)&h->d_b, 4 * (P + 1)));
  ORBFE_CREATE_HIP(h, orbfe_covis_destroy, hipMalloc((void**)&h->d_c, 4 * (P + 1)));
  ORBFE_CREATE_HIP(h, orbfe_covis_destroy, hipMalloc((void**)&h->d_tops, 4 * 4096));
  ORBFE_CREATE_HIP(h, orbfe_covis_destroy, hipMalloc((void**)&h->d_id_rank_of_row, 4 * M));
  ORBFE_CREATE_HIP(h, orbfe_covis_destroy, hipMalloc((void**)&h->d_tie_of_idrank, 2 * M));
  ORBFE_CREATE_HIP(h, orbfe_covis_destroy, hipMalloc((void**)&h->d_is_local, M));
  ORBFE_CREATE_HIP(h, orbfe_covis_destroy, hipMalloc((void**)&h->d_seen, 4 * M));
  ORBFE_CREATE_HIP(h, orbfe_covis_destroy, hipMalloc((void**)&h->d_order, 4 * M));
  ORBFE_CREATE_HIP(h, orbfe_covis_destroy, hipMalloc((void**)&h->d_attr, M * S));
  ORBFE_CREATE_HIP(h, orbfe_covis_destroy, hipMalloc((void**)&h->d_row_at_idrank, 4 * M));
  ORBFE_CREATE_HIP(h, orbfe_covis_destroy, hipMalloc((void**)&h->d_culled, 4 * M));
  ORBFE_CREATE_HIP(h, orbfe_covis_destroy, hipMemsetAsync(h->d_row_at_idrank, 0, 4 * M, h->stream));
  ORBFE_CREATE_HIP(h, orbfe_covis_destroy, hipMemsetAsync(h->d_row_n, 0xff, 4 * M, h->stream));
  ORBFE_CREATE_HIP(h, orbfe_covis_destroy, hipMemsetAsync(h->d_bad, 0, P, h->stream));
  ORBFE_CREATE_HIP(h, orbfe_covis_destroy, hipMemsetAsync(h->d_a, 0, 4 * (P + 1), h->stream));
  ORBFE_CREATE_HIP(h, orbfe_covis_destroy, hipMemsetAsync(h->d_id_rank_of_row, 0, 4 * M, h->stream));
  ORBFE_CREATE_HIP(h, orbfe_covis_destroy, hipMemsetAsync(h->d_tie_of_idrank, 0, 2 * M, h->stream));
  ORBFE_CREATE_HIP(h, orbfe_covis_destroy, hipStreamSynchronize(h->stream));
  *out = h;
  return ORBFE_OK;
}

extern "C" int orbfe_covis_destroy(orbfe_covis* h) {
  if (!h) return ORBFE_OK;
  if (orbfe_dev_close(h)) {
    hipFree(h->d_rows);
    hipFree(h->d_row_n);
    hipFree(h->d_bad);
    hipFree(h->d_a);
    hipFree(h->d_b);
    hipFree(h->d_c);
    hipFree(h->d_tops);
    hipFree(h->d_id_rank_of_row);
    hipFree(h->d_tie_of_idrank);
    hipFree(h->d_is_local);
    hipFree(h->d_seen);
    hipFree(h->d_order);
    hipFree(h->d_attr);
    hipFree(h->d_row_at_idrank);
    hipFree(h->d_culled);
    hipFree(h->d_tmp);
    hipFree(h->d_obs);
    hipFree(h->d_stage);
    hipFree(h->d_res);
    hipFree(h->d_lm_first);
    hipFree(h->d_geo_rec);
    hipFree(h->d_geo_state);
    hipFree(h->d_geo_out);
    if (h->h_stage) hipHostFree(h->h_stage);
    if (h->h_res) hipHostFree(h->h_res);
  }
  delete h;
  return ORBFE_OK;
}

extern "C" int orbfe_covis_set_keyframe(orbfe_covis* h, int64_t kf_id, uint64_t tie_key, int n_slots,
                                        const int32_t* point_ids) {
  if (!h) return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_covis_set_keyframe: bad argument");
  int row = -1, top = 0;
  cc::Status cs = h->core.prepare_keyframe(kf_id, tie_key, n_slots, point_ids, &row, &top);
  if (cs) return covis_fail("orbfe_covis_set_keyframe", cs);
  if (h->device >= 0) {
    hipSetDevice(h->device);
    int st = covis_stage_reserve(h, orbfe_al256(4 * (size_t)n_slots) + 256);
    if (st) return st;
    st = covis_upload(h, point_ids, 4 * (size_t)n_slots, h->d_rows + (size_t)row * h->core.S, nullptr);
    if (st) return st;
    const int32_t n32 = n_slots;
    st = covis_upload(h, &n32, 4, h->d_row_n + row, nullptr);
    if (st) return st;
    ORBFE_HIP_CHECK(hipStreamSynchronize(h->stream));
  }
  h->core.commit_keyframe(row, kf_id, tie_key, n_slots, top);
  return ORBFE_OK;
}

extern "C" int orbfe_covis_set_slots(orbfe_covis* h, int64_t kf_id, int n, const int32_t* slots,
                                     const int32_t* point_ids) {
  if (!h) return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_covis_set_slots: bad argument");
  int row = -1, top = 0;
  cc::Status cs = h->core.prepare_slots(kf_id, n, slots, point_ids, &row, &h->tmp_slots, &h->tmp_ids, &top);
  if (cs) return covis_fail("orbfe_covis_set_slots", cs);
  const int m = (int)h->tmp_slots.size();
  if (h->device >= 0 && m > 0) {
    hipSetDevice(h->device);
    int st = covis_stage_reserve(h, 2 * orbfe_al256(4 * (size_t)m));
    if (st) return st;
    const void *d_slots, *d_ids;
    st = covis_upload(h, h->tmp_slots.data(), 4 * (size_t)m, nullptr, &d_slots);
    if (st) return st;
    st = covis_upload(h, h->tmp_ids.data(), 4 * (size_t)m, nullptr, &d_ids);
    if (st) return st;
    ORBFE_LAUNCH("k_covis_scatter", k_covis_scatter, dim3((m + COVIS_ROW_THREADS - 1) / COVIS_ROW_THREADS),
                 dim3(COVIS_ROW_THREADS), 0, h->stream, h->d_rows + (size_t)row * h->core.S, h->core.row_n[row], m,
                 (const int32_t*)d_slots, (const int32_t*)d_ids);
    ORBFE_HIP_CHECK(hipGetLastError());
    ORBFE_HIP_CHECK(hipStreamSynchronize(h->stream));
  }
  h->core.commit_slots(m, top);
  return ORBFE_OK;
}

extern "C" int orbfe_covis_erase_keyframe(orbfe_covis* h, int64_t kf_id) {
  if (!h) return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_covis_erase_keyframe: bad argument");
  if (h->device >= 0 && h->core.slot_of.count(kf_id)) {
    hipSetDevice(h->device);
    ORBFE_HIP_CHECK(hipMemsetAsync(h->d_row_n + h->core.slot_of[kf_id], 0xff, 4, h->stream));
    ORBFE_HIP_CHECK(hipStreamSynchronize(h->stream));
  }
  int row = -1;
  cc::Status cs = h->core.erase(kf_id, &row);
  if (cs) return covis_fail("orbfe_covis_erase_keyframe", cs);
  return ORBFE_OK;
}

extern "C" int orbfe_covis_set_points_bad(orbfe_covis* h, int n, const int32_t* point_ids, int bad) {
  if (!h || n < 0 || (n > 0 && !point_ids))
    return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_covis_set_points_bad: bad argument");
  int top = 0;
  cc::Status cs = h->core.check_points(n, point_ids, &top);
  if (cs) return covis_fail("orbfe_covis_set_points_bad", cs);
  for (int i = 0; i < n; i++)
    if (point_ids[i] < 0) return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_covis_set_points_bad: a point id below 0");
  if (h->device >= 0 && n > 0) {
    hipSetDevice(h->device);
    int st = covis_stage_reserve(h, orbfe_al256(4 * (size_t)n));
    if (st) return st;
    const void* d_ids;
    st = covis_upload(h, point_ids, 4 * (size_t)n, nullptr, &d_ids);
    if (st) return st;
    ORBFE_LAUNCH("k_covis_set_bad", k_covis_set_bad, dim3((n + COVIS_ROW_THREADS - 1) / COVIS_ROW_THREADS),
                 dim3(COVIS_ROW_THREADS), 0, h->stream, h->d_bad, h->core.P, n, (const int32_t*)d_ids, bad ? 1 : 0);
    ORBFE_HIP_CHECK(hipGetLastError());
    ORBFE_HIP_CHECK(hipStreamSynchronize(h->stream));
  }
  return ORBFE_OK;
}

extern "C" int orbfe_covis_clear(orbfe_covis* h) {
  if (!h) return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_covis_clear: bad argument");
  if (h->device >= 0) {
    hipSetDevice(h->device);
    ORBFE_HIP_CHECK(hipMemsetAsync(h->d_row_n, 0xff, 4 * (size_t)h->core.M, h->stream));
    ORBFE_HIP_CHECK(hipMemsetAsync(h->d_bad, 0, (size_t)h->core.P, h->stream));
    if (h->d_geo_state) ORBFE_HIP_CHECK(hipMemsetAsync(h->d_geo_state, 0, (size_t)h->core.P, h->stream));
    ORBFE_HIP_CHECK(hipStreamSynchronize(h->stream));
  }
  h->core.clear();
  return ORBFE_OK;
}

extern "C" int orbfe_covis_size(const orbfe_covis* h, int* n) {
  if (!h || !n) return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_covis_size: bad argument");
  *n = h->core.size();
  return ORBFE_OK;
}

// data[0..n) -> exclusive scan in place, data[n] = the total (n >= 1)
static void covis_scan(orbfe_covis* h, int32_t* data, int n) {
  const int nb = (n + COVIS_SCAN_TILE - 1) / COVIS_SCAN_TILE;
  ORBFE_LAUNCH("k_covis_scan_local", k_covis_scan_local, dim3(nb), dim3(COVIS_THREADS), 0, h->stream, data, n,
               h->d_tops);
  ORBFE_LAUNCH("k_covis_scan_tops", k_covis_scan_tops, dim3(1), dim3(COVIS_THREADS), 0, h->stream, h->d_tops, nb,
               data + n);
  if (nb > 1)
    ORBFE_LAUNCH("k_covis_scan_add", k_covis_scan_add, dim3(nb), dim3(COVIS_THREADS), 0, h->stream, data, n,
                 (const int32_t*)h->d_tops);
}

static CovisTable covis_table(const orbfe_covis* h) {
  CovisTable t;
  t.rows = h->d_rows;
  t.row_n = h->d_row_n;
  t.bad = h->d_bad;
  t.begin = h->d_a;
  t.obs = h->d_obs;
  t.S = h->core.S;
  t.n_pts = h->core.p_hi;
  t.n_live = h->core.size();
  return t;
}

static size_t covis_refresh_bytes(const orbfe_covis* h) {
  return 2 * orbfe_al256(4 * (size_t)h->core.M) + orbfe_al256(2 * (size_t)h->core.M);
}

static int covis_max_row(const orbfe_covis* h) {
  int m = 0;
  for (int k = 0; k < h->core.hi; k++) m = std::max(m, h->core.row_n[k]);
  return m;
}

// The rank tables and the inverse as of now, enqueued on the stream (the staging has room).
static int covis_refresh(orbfe_covis* h) {
  cc::Core& c = h->core;
  if (c.ranks_dirty) {
    c.ranks();
    int st = covis_upload(h, c.id_rank_of_row.data(), 4 * c.id_rank_of_row.size(), h->d_id_rank_of_row, nullptr);
    if (st) return st;
    st = covis_upload(h, c.tie_rank_of_id_rank.data(), 2 * c.tie_rank_of_id_rank.size(), h->d_tie_of_idrank, nullptr);
    if (st) return st;
    st = covis_upload(h, c.row_at_id_rank.data(), 4 * c.row_at_id_rank.size(), h->d_row_at_idrank, nullptr);
    if (st) return st;
    c.stale = true;  // inverse entries carry mnId ranks
  }
  if (!c.stale) return ORBFE_OK;
  const int n_pts = c.p_hi;
  ORBFE_HIP_CHECK(hipMemsetAsync(h->d_a, 0, 4 * ((size_t)n_pts + 1), h->stream));
  const int max_row = covis_max_row(h);
  if (n_pts > 0 && c.total_slots > 0 && max_row > 0) {
    if (c.total_slots > h->obs_cap) {
      ORBFE_HIP_CHECK(hipStreamSynchronize(h->stream));
      hipFree(h->d_tmp);
      hipFree(h->d_obs);
      h->d_tmp = nullptr;
      h->d_obs = nullptr;
      h->obs_cap = 0;
      const long long cap = std::min<long long>(c.total_slots + c.total_slots / 2 + 1024, (long long)c.M * c.S);
      ORBFE_HIP_CHECK(hipMalloc((void**)&h->d_tmp, 8 * (size_t)cap));
      ORBFE_HIP_CHECK(hipMalloc((void**)&h->d_obs, 4 * (size_t)cap));
      h->obs_cap = cap;
    }
    ORBFE_HIP_CHECK(hipMemsetAsync(h->d_c, 0, 4 * ((size_t)n_pts + 1), h->stream));
    const CovisTable t = covis_table(h);
    const dim3 grid((max_row + COVIS_ROW_THREADS - 1) / COVIS_ROW_THREADS, c.hi);
    ORBFE_LAUNCH("k_covis_count", k_covis_count, grid, dim3(COVIS_ROW_THREADS), 0, h->stream, t, h->d_a);
    covis_scan(h, h->d_a, n_pts);
    ORBFE_LAUNCH("k_covis_fill", k_covis_fill, grid, dim3(COVIS_ROW_THREADS), 0, h->stream, t, h->d_c,
                 (const int32_t*)h->d_id_rank_of_row, h->d_tmp, h->obs_cap);
    const long long nb = (c.total_slots + COVIS_ROW_THREADS - 1) / COVIS_ROW_THREADS;
    ORBFE_LAUNCH("k_covis_canon", k_covis_canon, dim3((unsigned)nb), dim3(COVIS_ROW_THREADS), 0, h->stream, t,
                 (const unsigned long long*)h->d_tmp, h->obs_cap);
    ORBFE_HIP_CHECK(hipGetLastError());
  }
  c.stale = false;
  return ORBFE_OK;
}

// The vote kernel over n queries (rows, or point lists), the packed result in h_res after one
// synchronisation: per query 4 + 2 * stride words.
static int covis_run_votes(orbfe_covis* h, int n, const int32_t* d_rows, const int32_t* d_self,
                           const int32_t* d_begin, const int32_t* d_points, int th, int want_ordered, int stride) {
  const size_t bytes = 4 * (size_t)n * (4 + 2 * (size_t)stride);
  int st = covis_res_reserve(h, bytes);
  if (st) return st;
  CovisVoteArgs a;
  a.t = covis_table(h);
  a.tie_of_idrank = h->d_tie_of_idrank;
  a.q_row = d_rows;
  a.q_self = d_self;
  a.q_begin = d_begin;
  a.q_points = d_points;
  a.th = th;
  a.want_ordered = want_ordered;
  a.stride = stride;
  a.out = reinterpret_cast<uint32_t*>(h->d_res);
  ORBFE_LAUNCH("k_covis_vote", k_covis_vote, dim3(n), dim3(COVIS_THREADS), 0, h->stream, a);
  ORBFE_HIP_CHECK(hipGetLastError());
  ORBFE_HIP_CHECK(hipMemcpyAsync(h->h_res, h->d_res, bytes, hipMemcpyDeviceToHost, h->stream));
  ORBFE_HIP_CHECK(hipStreamSynchronize(h->stream));
  return ORBFE_OK;
}

extern "C" int orbfe_covis_update_connections(orbfe_covis* h, int n, const int64_t* kf_ids, int th,
                                              orbfe_covis_connections_t* r) {
  if (!h || !r || r->capacity < 0 ||
      (n > 0 && (!r->n_counter || !r->n_ordered || !r->nmax || !r->kf_max || !r->unchanged)) ||
      (n > 0 && r->capacity > 0 &&
       (!r->counter_ids || !r->counter_weights || !r->ordered_ids || !r->ordered_weights)))
    return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_covis_update_connections: bad argument");
  cc::Status cs = h->core.rows_of(n, kf_ids, &h->tmp_rows);
  if (cs) return covis_fail("orbfe_covis_update_connections", cs);
  if (h->device < 0) return orbfe_set_error(ORBFE_ERR_STATE, "covisibility table is host-only (device < 0)");
  if (n == 0) return ORBFE_OK;
  hipSetDevice(h->device);
  int st = covis_stage_reserve(h, covis_refresh_bytes(h) + 2 * orbfe_al256(4 * (size_t)n));
  if (st) return st;
  st = covis_refresh(h);
  if (st) return st;
  const cc::Core& c = h->core;
  std::vector<int32_t> self(n);
  for (int i = 0; i < n; i++) self[i] = c.tie_rank_of_row[h->tmp_rows[i]];
  const void *d_rows, *d_self;
  st = covis_upload(h, h->tmp_rows.data(), 4 * (size_t)n, nullptr, &d_rows);
  if (st) return st;
  st = covis_upload(h, self.data(), 4 * (size_t)n, nullptr, &d_self);
  if (st) return st;
  const int stride = std::max(std::min(r->capacity, c.size() - 1), 0);
  st = covis_run_votes(h, n, (const int32_t*)d_rows, (const int32_t*)d_self, nullptr, nullptr, th, 1, stride);
  if (st) return st;
  const uint32_t* res = reinterpret_cast<const uint32_t*>(h->h_res);
  const size_t per = 4 + 2 * (size_t)stride;
  const int live = c.size();
  for (int q = 0; q < n; q++) {
    const uint32_t* o = res + q * per;
    bool sane = (int)o[0] <= live && (int)o[1] <= live && (o[0] == 0 || (int)(o[3] & 4095u) < live);
    for (int i = 0; sane && i < std::min((int)o[0], stride); i++) sane = cc::key_rank(o[4 + i]) < live;
    for (int i = 0; sane && i < std::min((int)o[1], stride); i++) sane = cc::key_rank(o[4 + stride + i]) < live;
    if (!sane) return orbfe_set_error(ORBFE_ERR_STATE, "orbfe_covis_update_connections: corrupt result");
    if ((int)o[0] > r->capacity || (int)o[1] > r->capacity)
      return orbfe_set_error(ORBFE_ERR_CAPACITY, "orbfe_covis_update_connections: result capacity below a counter");
  }
  for (int q = 0; q < n; q++) {
    const uint32_t* o = res + q * per;
    const int nc = (int)o[0], no = (int)o[1];
    const size_t base = (size_t)q * r->capacity;
    r->n_counter[q] = nc;
    r->n_ordered[q] = no;
    r->nmax[q] = (int32_t)o[2];
    r->kf_max[q] = nc > 0 ? c.id_of[c.row_at_tie_rank[o[3] & 4095u]] : -1;
    r->unchanged[q] = nc == 0 ? 1 : 0;
    for (int i = 0; i < nc; i++) {
      r->counter_ids[base + i] = c.id_of[c.row_at_tie_rank[cc::key_rank(o[4 + i])]];
      r->counter_weights[base + i] = cc::key_weight(o[4 + i]);
    }
    for (int i = 0; i < no; i++) {
      r->ordered_ids[base + i] = c.id_of[c.row_at_tie_rank[cc::key_rank(o[4 + stride + i])]];
      r->ordered_weights[base + i] = cc::key_weight(o[4 + stride + i]);
    }
  }
  return ORBFE_OK;
}

extern "C" int orbfe_covis_vote(orbfe_covis* h, int n_queries, const int32_t* begin, const int32_t* point_ids,
                                orbfe_covis_votes_t* r) {
  if (!h || !r || r->capacity < 0 || (n_queries > 0 && (!r->n || !r->max || !r->kf_max)) ||
      (n_queries > 0 && r->capacity > 0 && (!r->kf_ids || !r->counts)))
    return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_covis_vote: bad argument");
  cc::Status cs = h->core.check_votes(n_queries, begin, point_ids);
  if (cs) return covis_fail("orbfe_covis_vote", cs);
  if (h->device < 0) return orbfe_set_error(ORBFE_ERR_STATE, "covisibility table is host-only (device < 0)");
  if (n_queries == 0) return ORBFE_OK;
  hipSetDevice(h->device);
  const int total = begin[n_queries];
  int st = covis_stage_reserve(h, covis_refresh_bytes(h) + orbfe_al256(4 * ((size_t)n_queries + 1)) +
                                      orbfe_al256(4 * (size_t)total));
  if (st) return st;
  st = covis_refresh(h);
  if (st) return st;
  const cc::Core& c = h->core;
  const void *d_begin, *d_points;
  st = covis_upload(h, begin, 4 * ((size_t)n_queries + 1), nullptr, &d_begin);
  if (st) return st;
  st = covis_upload(h, point_ids, 4 * (size_t)total, nullptr, &d_points);
  if (st) return st;
  const int stride = std::min(r->capacity, c.size());
  st = covis_run_votes(h, n_queries, nullptr, nullptr, (const int32_t*)d_begin, (const int32_t*)d_points, 0, 0,
                       stride);
  if (st) return st;
  const uint32_t* res = reinterpret_cast<const uint32_t*>(h->h_res);
  const size_t per = 4 + 2 * (size_t)stride;
  for (int q = 0; q < n_queries; q++) {
    const int nc = (int)res[q * per];
    bool sane = nc >= 0 && nc <= c.size() && (nc == 0 || (int)(res[q * per + 3] & 4095u) < c.size());
    for (int i = 0; sane && i < std::min(nc, stride); i++) sane = cc::key_rank(res[q * per + 4 + i]) < c.size();
    if (!sane) return orbfe_set_error(ORBFE_ERR_STATE, "orbfe_covis_vote: corrupt result");
    if (nc > r->capacity) return orbfe_set_error(ORBFE_ERR_CAPACITY, "orbfe_covis_vote: result capacity below a counter");
  }
  for (int q = 0; q < n_queries; q++) {
    const uint32_t* o = res + q * per;
    const int nc = (int)o[0];
    const size_t base = (size_t)q * r->capacity;
    r->n[q] = nc;
    r->max[q] = (int32_t)o[2];
    r->kf_max[q] = nc > 0 ? c.id_of[c.row_at_tie_rank[o[3] & 4095u]] : -1;
    for (int i = 0; i < nc; i++) {
      r->kf_ids[base + i] = c.id_of[c.row_at_tie_rank[cc::key_rank(o[4 + i])]];
      r->counts[base + i] = cc::key_weight(o[4 + i]);
    }
  }
  return ORBFE_OK;
}

extern "C" int orbfe_covis_local_map(orbfe_covis* h, int n_local, const int64_t* local_kf_ids,
                                     orbfe_covis_local_map_t* r) {
  if (!h || !r || r->point_capacity < 0 || r->fixed_capacity < 0 || r->edge_capacity < 0 || !r->edge_begin ||
      (r->point_capacity > 0 && !r->point_ids) || (r->fixed_capacity > 0 && !r->fixed_ids) ||
      (r->edge_capacity > 0 && (!r->edge_kf || !r->edge_slot)))
    return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_covis_local_map: bad argument");
  cc::Status cs = h->core.local_rows(n_local, local_kf_ids, &h->tmp_rows);
  if (cs) return covis_fail("orbfe_covis_local_map", cs);
  if (h->device < 0) return orbfe_set_error(ORBFE_ERR_STATE, "covisibility table is host-only (device < 0)");
  r->n_points = r->n_fixed = r->n_edges = 0;
  r->edge_begin[0] = 0;
  if (n_local == 0) return ORBFE_OK;
  hipSetDevice(h->device);
  cc::Core& c = h->core;
  int st = covis_stage_reserve(h, covis_refresh_bytes(h) + orbfe_al256(4 * (size_t)n_local) + orbfe_al256((size_t)c.M));
  if (st) return st;
  st = covis_refresh(h);
  if (st) return st;
  const int n_pts = c.p_hi, live = c.size();
  const int max_row = covis_max_row(h);
  if (n_pts == 0 || max_row == 0) {  // no row holds a point
    ORBFE_HIP_CHECK(hipStreamSynchronize(h->stream));  // the refresh read the staging
    return ORBFE_OK;
  }
  std::vector<uint8_t> is_local(live, 0);
  for (int i = 0; i < n_local; i++) is_local[c.id_rank_of_row[h->tmp_rows[i]]] = 1;
  const void* d_local;
  st = covis_upload(h, h->tmp_rows.data(), 4 * (size_t)n_local, nullptr, &d_local);
  if (st) return st;
  st = covis_upload(h, is_local.data(), (size_t)live, h->d_is_local, nullptr);
  if (st) return st;
  const int pt_cap = std::min(r->point_capacity, n_pts);
  const int fx_cap = std::min(r->fixed_capacity, live);
  const int ed_cap = (int)std::min<long long>(r->edge_capacity, c.total_slots);
  // result: hdr[4] | points[pt_cap] | ebeg[pt_cap + 1] | fixed[fx_cap] | edge_kf[ed_cap] | edge_slot[ed_cap]
  const size_t o_pts = 4, o_ebeg = o_pts + pt_cap, o_fix = o_ebeg + pt_cap + 1, o_ekf = o_fix + fx_cap,
               o_esl = o_ekf + ed_cap, words = o_esl + ed_cap;
  st = covis_res_reserve(h, 4 * words);
  if (st) return st;
  int32_t* d = reinterpret_cast<int32_t*>(h->d_res);
  int32_t* hres = reinterpret_cast<int32_t*>(h->h_res);
  const CovisTable t = covis_table(h);
  ORBFE_HIP_CHECK(hipMemsetAsync(d, 0, 16, h->stream));
  ORBFE_HIP_CHECK(hipMemsetAsync(h->d_b, 0, 4 * ((size_t)n_pts + 1), h->stream));
  ORBFE_HIP_CHECK(hipMemsetAsync(h->d_seen, 0, 4 * (size_t)live, h->stream));
  ORBFE_LAUNCH("k_covis_lm_mark", k_covis_lm_mark,
               dim3((max_row + COVIS_ROW_THREADS - 1) / COVIS_ROW_THREADS, n_local), dim3(COVIS_ROW_THREADS), 0,
               h->stream, t, (const int32_t*)d_local, h->d_b);
  const int pb = (n_pts + COVIS_ROW_THREADS - 1) / COVIS_ROW_THREADS;
  ORBFE_LAUNCH("k_covis_lm_count", k_covis_lm_count, dim3(pb), dim3(COVIS_ROW_THREADS), 0, h->stream, t,
               (const int32_t*)h->d_b, h->d_c);
  covis_scan(h, h->d_b, n_pts);
  covis_scan(h, h->d_c, n_pts);
  CovisEmitArgs ea;
  ea.t = t;
  ea.pidx = h->d_b;
  ea.ebeg = h->d_c;
  ea.pt_cap = pt_cap;
  ea.edge_cap = ed_cap;
  ea.hdr = d;
  ea.out_points = d + o_pts;
  ea.out_ebeg = d + o_ebeg;
  ea.edge_kf = d + o_ekf;
  ea.edge_slot = d + o_esl;
  ea.seen = h->d_seen;
  ORBFE_LAUNCH("k_covis_lm_emit", k_covis_lm_emit, dim3(pb), dim3(COVIS_ROW_THREADS), 0, h->stream, ea);
  ORBFE_LAUNCH("k_covis_lm_order", k_covis_lm_order, dim3(1), dim3(COVIS_THREADS), 0, h->stream, live, n_local,
               (const uint8_t*)h->d_is_local, (const int32_t*)h->d_seen, h->d_order, fx_cap, d + o_fix, d);
  if (ed_cap > 0)
    ORBFE_LAUNCH("k_covis_lm_edges", k_covis_lm_edges, dim3((ed_cap + COVIS_ROW_THREADS - 1) / COVIS_ROW_THREADS),
                 dim3(COVIS_ROW_THREADS), 0, h->stream, (const int32_t*)d, ed_cap, live, (const int32_t*)h->d_order,
                 d + o_ekf);
  ORBFE_HIP_CHECK(hipGetLastError());
  ORBFE_HIP_CHECK(hipMemcpyAsync(hres, d, 16, hipMemcpyDeviceToHost, h->stream));
  ORBFE_HIP_CHECK(hipStreamSynchronize(h->stream));
  const int np = hres[0], ne = hres[1], nf = hres[2];
  if (np < 0 || np > n_pts || ne < 0 || ne > c.total_slots || nf < 0 || nf > live)
    return orbfe_set_error(ORBFE_ERR_STATE, "orbfe_covis_local_map: corrupt result");
  if (np > r->point_capacity || nf > r->fixed_capacity || ne > r->edge_capacity) {
    r->n_points = np;
    r->n_fixed = nf;
    r->n_edges = ne;
    return orbfe_set_error(ORBFE_ERR_CAPACITY, "orbfe_covis_local_map: a result capacity below what the gather found");
  }
  ORBFE_HIP_CHECK(hipMemcpyAsync(hres + o_pts, d + o_pts, 4 * (size_t)np, hipMemcpyDeviceToHost, h->stream));
  ORBFE_HIP_CHECK(hipMemcpyAsync(hres + o_ebeg, d + o_ebeg, 4 * ((size_t)np + 1), hipMemcpyDeviceToHost, h->stream));
  ORBFE_HIP_CHECK(hipMemcpyAsync(hres + o_fix, d + o_fix, 4 * (size_t)nf, hipMemcpyDeviceToHost, h->stream));
  ORBFE_HIP_CHECK(hipMemcpyAsync(hres + o_ekf, d + o_ekf, 4 * (size_t)ne, hipMemcpyDeviceToHost, h->stream));
  ORBFE_HIP_CHECK(hipMemcpyAsync(hres + o_esl, d + o_esl, 4 * (size_t)ne, hipMemcpyDeviceToHost, h->stream));
  ORBFE_HIP_CHECK(hipStreamSynchronize(h->stream));
  r->n_points = np;
  r->n_fixed = nf;
  r->n_edges = ne;
  if (np > 0) memcpy(r->point_ids, hres + o_pts, 4 * (size_t)np);
  memcpy(r->edge_begin, hres + o_ebeg, 4 * ((size_t)np + 1));
  for (int i = 0; i < nf; i++) {
    const int rank = hres[o_fix + i];
    if (rank < 0 || rank >= live) return orbfe_set_error(ORBFE_ERR_STATE, "orbfe_covis_local_map: corrupt result");
    r->fixed_ids[i] = c.id_of[c.row_at_id_rank[rank]];
  }
  if (ne > 0) {
    memcpy(r->edge_kf, hres + o_ekf, 4 * (size_t)ne);
    memcpy(r->edge_slot, hres + o_esl, 4 * (size_t)ne);
  }
  return ORBFE_OK;
}

extern "C" int orbfe_covis_set_keyframe_attrs(orbfe_covis* h, int64_t kf_id, int n_slots, const uint8_t* attrs) {
  if (!h) return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_covis_set_keyframe_attrs: bad argument");
  int row = -1;
  cc::Status cs = h->core.prepare_attrs(kf_id, n_slots, attrs, &row);
  if (cs) return covis_fail("orbfe_covis_set_keyframe_attrs", cs);
  if (h->device >= 0 && n_slots > 0) {
    hipSetDevice(h->device);
    int st = covis_stage_reserve(h, orbfe_al256((size_t)n_slots));
    if (st) return st;
    st = covis_upload(h, attrs, (size_t)n_slots, h->d_attr + (size_t)row * h->core.S, nullptr);
    if (st) return st;
    ORBFE_HIP_CHECK(hipStreamSynchronize(h->stream));
  }
  h->core.commit_attrs(row);
  return ORBFE_OK;
}

static CovisCullArgs covis_cull_args(const orbfe_covis* h) {
  CovisCullArgs a;
  memset(&a, 0, sizeof(a));
  a.t = covis_table(h);
  a.M = h->core.M;
  a.attr = h->d_attr;
  a.row_at_idrank = h->d_row_at_idrank;
  a.id_rank_of_row = h->d_id_rank_of_row;
  return a;
}

extern "C" int orbfe_covis_cull_keyframes(orbfe_covis* h, int n, const int64_t* kf_ids, const uint8_t* not_erase,
                                          int monocular, orbfe_covis_cull_t* r) {
  if (!h || !r || !r->bad_begin || r->bad_capacity < 0 || (r->bad_capacity > 0 && !r->bad_points) ||
      (n > 0 && (!r->decision || !r->n_mps || !r->n_redundant)))
    return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_covis_cull_keyframes: bad argument");
  cc::Status cs = h->core.prepare_cull(n, kf_ids, not_erase, r->bad_capacity, &h->tmp_rows);
  if (cs) return covis_fail("orbfe_covis_cull_keyframes", cs);
  if (h->device < 0) return orbfe_set_error(ORBFE_ERR_STATE, "covisibility table is host-only (device < 0)");
  r->bad_begin[0] = 0;
  if (n == 0) return ORBFE_OK;
  hipSetDevice(h->device);
  cc::Core& c = h->core;
  int st = covis_stage_reserve(h, covis_refresh_bytes(h) + orbfe_al256(4 * (size_t)n) + orbfe_al256((size_t)n));
  if (st) return st;
  st = covis_refresh(h);
  if (st) return st;
  std::vector<uint8_t> flag(n);
  int64_t need = 0;
  for (int i = 0; i < n; i++) {
    flag[i] = (uint8_t)((not_erase[i] ? 1 : 0) | (kf_ids[i] == 0 ? 2 : 0));
    need += c.row_n[h->tmp_rows[i]];
  }
  const void *d_rows, *d_flag;
  st = covis_upload(h, h->tmp_rows.data(), 4 * (size_t)n, nullptr, &d_rows);
  if (st) return st;
  st = covis_upload(h, flag.data(), (size_t)n, nullptr, &d_flag);
  if (st) return st;
  // result words: round_min[n + 1] | cursor | n_mps[n] | n_red[n] | bad_count[n] | bad_list[need] ; decision[n] bytes
  const size_t o_cur = (size_t)n + 1, o_mps = o_cur + 1, o_red = o_mps + n, o_cnt = o_red + n, o_list = o_cnt + n,
               o_dec = o_list + (size_t)need, bytes = 4 * o_dec + (size_t)n;
  st = covis_res_reserve(h, bytes);
  if (st) return st;
  int32_t* d = reinterpret_cast<int32_t*>(h->d_res);
  int32_t* hres = reinterpret_cast<int32_t*>(h->h_res);
  ORBFE_HIP_CHECK(hipMemsetAsync(d, 0x7f, 4 * ((size_t)n + 1), h->stream));
  ORBFE_HIP_CHECK(hipMemsetAsync(d + o_cur, 0, bytes - 4 * o_cur, h->stream));
  ORBFE_HIP_CHECK(hipMemsetAsync(h->d_culled, 0, 4 * (size_t)c.M, h->stream));
  CovisCullArgs a = covis_cull_args(h);
  a.culled = h->d_culled;
  a.cand_row = (const int32_t*)d_rows;
  a.cand_flag = (const uint8_t*)d_flag;
  a.n = n;
  a.monocular = monocular ? 1 : 0;
  a.decision = reinterpret_cast<uint8_t*>(d + o_dec);
  a.n_mps = d + o_mps;
  a.n_red = d + o_red;
  a.bad_count = d + o_cnt;
  a.bad_list = d + o_list;
  a.bad_cursor = d + o_cur;
  a.bad_cap = (int)need;
  std::vector<int> culled;
  int start = 0;
  // A round decides every candidate from `start` on against the culls so far; the lowest one that culls is
  // committed and the next round starts behind it. Rounds = culls + 1 at the most.
  for (int round = 0; round <= n && start < n; round++) {
    a.start = start;
    a.round_min = d + round;
    ORBFE_LAUNCH("k_covis_cull_eval", k_covis_cull_eval, dim3(n - start), dim3(COVIS_ROW_THREADS), 0, h->stream, a);
    ORBFE_LAUNCH("k_covis_cull_commit", k_covis_cull_commit, dim3(1), dim3(COVIS_THREADS), 0, h->stream, a);
    ORBFE_HIP_CHECK(hipGetLastError());
    ORBFE_HIP_CHECK(hipMemcpyAsync(hres + round, d + round, 4, hipMemcpyDeviceToHost, h->stream));
    ORBFE_HIP_CHECK(hipStreamSynchronize(h->stream));
    const int idx = hres[round];
    if (idx == COVIS_CULL_NONE) break;
    if (idx < start || idx >= n) {
      c.stale = true;
      return orbfe_set_error(ORBFE_ERR_STATE, "orbfe_covis_cull_keyframes: corrupt result");
    }
    culled.push_back(idx);
    start = idx + 1;
  }
  ORBFE_HIP_CHECK(hipMemcpyAsync(hres + o_cur, d + o_cur, bytes - 4 * o_cur, hipMemcpyDeviceToHost, h->stream));
  ORBFE_HIP_CHECK(hipStreamSynchronize(h->stream));
  // the table changed whatever follows
  for (int idx : culled) {
    int row = -1;
    c.erase(kf_ids[idx], &row);
  }
  bool sane = hres[o_cur] >= 0 && hres[o_cur] <= need;
  int64_t total = 0;
  for (int i = 0; sane && i < n; i++) {
    const int k = hres[o_cnt + i];
    sane = k >= 0 && total + k <= need;
    total += k;
  }
  sane = sane && total == hres[o_cur];
  for (int64_t i = 0; sane && i < total; i++) sane = hres[o_list + i] >= 0 && hres[o_list + i] < c.P;
  if (!sane) {
    c.stale = true;
    return orbfe_set_error(ORBFE_ERR_STATE, "orbfe_covis_cull_keyframes: corrupt result");
  }
  if (total > 0) c.stale = true;
  const uint8_t* dec = reinterpret_cast<const uint8_t*>(hres + o_dec);
  int32_t at = 0;
  for (int i = 0; i < n; i++) {
    r->decision[i] = dec[i];
    r->n_mps[i] = hres[o_mps + i];
    r->n_redundant[i] = hres[o_red + i];
    r->bad_begin[i] = at;
    at += hres[o_cnt + i];
  }
  r->bad_begin[n] = at;
  if (total > 0) memcpy(r->bad_points, hres + o_list, 4 * (size_t)total);
  return ORBFE_OK;
}

extern "C" int orbfe_covis_cull_points(orbfe_covis* h, int n, const int32_t* point_ids, const int32_t* found,
                                       const int32_t* visible, const int64_t* first_kf_id, int64_t current_kf_id,
                                       int monocular, uint8_t* action) {
  if (!h) return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_covis_cull_points: bad argument");
  cc::Status cs = h->core.prepare_cull_points(n, point_ids, found, visible, first_kf_id, current_kf_id, action);
  if (cs) return covis_fail("orbfe_covis_cull_points", cs);
  if (h->device < 0) return orbfe_set_error(ORBFE_ERR_STATE, "covisibility table is host-only (device < 0)");
  if (n == 0) return ORBFE_OK;
  hipSetDevice(h->device);
  cc::Core& c = h->core;
  int st = covis_stage_reserve(h, covis_refresh_bytes(h) + 3 * orbfe_al256(4 * (size_t)n) + orbfe_al256(8 * (size_t)n));
  if (st) return st;
  st = covis_refresh(h);
  if (st) return st;
  const void *d_ids, *d_found, *d_vis, *d_first;
  st = covis_upload(h, point_ids, 4 * (size_t)n, nullptr, &d_ids);
  if (st) return st;
  st = covis_upload(h, found, 4 * (size_t)n, nullptr, &d_found);
  if (st) return st;
  st = covis_upload(h, visible, 4 * (size_t)n, nullptr, &d_vis);
  if (st) return st;
  st = covis_upload(h, first_kf_id, 8 * (size_t)n, nullptr, &d_first);
  if (st) return st;
  st = covis_res_reserve(h, (size_t)n);
  if (st) return st;
  CovisCullPointsArgs q;
  q.a = covis_cull_args(h);
  q.a.monocular = monocular ? 1 : 0;
  q.n_points = n;
  q.ids = (const int32_t*)d_ids;
  q.found = (const int32_t*)d_found;
  q.visible = (const int32_t*)d_vis;
  q.first = (const long long*)d_first;
  q.current = current_kf_id;
  q.action = h->d_res;
  q.P = c.P;
  ORBFE_HIP_CHECK(hipMemsetAsync(h->d_res, 0xff, (size_t)n, h->stream));
  ORBFE_LAUNCH("k_covis_cull_points", k_covis_cull_points, dim3((n + COVIS_ROW_THREADS - 1) / COVIS_ROW_THREADS),
               dim3(COVIS_ROW_THREADS), 0, h->stream, q);
  ORBFE_HIP_CHECK(hipGetLastError());
  ORBFE_HIP_CHECK(hipMemcpyAsync(h->h_res, h->d_res, (size_t)n, hipMemcpyDeviceToHost, h->stream));
  ORBFE_HIP_CHECK(hipStreamSynchronize(h->stream));
  bool changed = false;
  for (int i = 0; i < n; i++) {
    if (h->h_res[i] > CULL_PT_AGE) {
      c.stale = true;
      return orbfe_set_error(ORBFE_ERR_STATE, "orbfe_covis_cull_points: corrupt result");
    }
    changed = changed || h->h_res[i] == CULL_PT_RATIO || h->h_res[i] == CULL_PT_OBS;
  }
  if (changed) c.stale = true;
  memcpy(action, h->h_res, (size_t)n);
  return ORBFE_OK;
}

// ---- the local map (include/orbfe_localmap.h; orbfe_localmap_core.h holds the index arithmetic) ----
// The three row passes run one thread per (list position, slot) on a grid (nbx, n_kf) of 256 threads, so
// workgroup lm_block(position, bx) covers 256 consecutive slots and the workgroups ascend in (position,
// slot): k_lm_first takes the minimum key per point, k_lm_count counts each workgroup's first occurrences,
// the scan kernels above turn the counts into offsets, k_lm_emit ranks the first occurrences inside the
// workgroup (ballot + four wave totals), writes the point at offset + rank and the tagged index back into
// first[p]. k_lm_gather: four lanes per result point, one 16-byte load and store each of the 64-byte
// record. k_lm_seen: one thread per entry of the Frame's list. k_lm_reset: first[p] over the result only.
// Guards: a list row against M, a slot against the row's length and S, a point id against P (first, bad,
// the store and its state all hold P entries), an output index against `bound` (the capacity of out and of
// the gathered arrays), a result index against hdr[0] and bound.
struct LmArgs {
  const int32_t* rows;       // [M * S]
  const int32_t* row_n;      // [M]
  const uint8_t* bad;        // [P]
  int M, S, P;
  const int32_t* list_rows;  // [n_kf] row per list position
  int n_kf, nbx, n_blocks;
  uint32_t* first;           // [P]
  int32_t* blk;              // [n_blocks + 1]
  int32_t* hdr;              // {n_points, n_missing, 0, 0}
  int32_t* out;              // [bound]
  int bound;
};

// the non-bad point in slot s of list position pos, or -1
__device__ __forceinline__ int lm_slot_point(const LmArgs& a, int pos, int s) {
  const int k = a.list_rows[pos];
  if ((unsigned)k >= (unsigned)a.M) return -1;
  if (s >= a.row_n[k] || s >= a.S) return -1;
  const int p = a.rows[(size_t)k * a.S + s];
  if ((unsigned)p >= (unsigned)a.P) return -1;
  return a.bad[p] ? -1 : p;
}

__global__ __launch_bounds__(COVIS_ROW_THREADS) void k_lm_first(LmArgs a) {
  const int pos = blockIdx.y, s = (int)(blockIdx.x * COVIS_ROW_THREADS + threadIdx.x);
  const int p = lm_slot_point(a, pos, s);
  if (p >= 0) atomicMin(&a.first[p], lm::lm_key(pos, s));
}

__global__ __launch_bounds__(COVIS_ROW_THREADS) void k_lm_count(LmArgs a) {
  __shared__ int s_w[COVIS_ROW_THREADS / 64];
  const int pos = blockIdx.y, s = (int)(blockIdx.x * COVIS_ROW_THREADS + threadIdx.x);
  const int p = lm_slot_point(a, pos, s);
  const bool win = p >= 0 && a.first[p] == lm::lm_key(pos, s);
  const uint64_t m = wave_ballot(win);
  if (lane_id() == 0) s_w[wave_id()] = __popcll(m);
  __syncthreads();
  const int b = lm::lm_block(pos, blockIdx.x, a.nbx);
  if (threadIdx.x == 0 && b < a.n_blocks) a.blk[b] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

__global__ __launch_bounds__(COVIS_ROW_THREADS) void k_lm_emit(LmArgs a) {
  __shared__ int s_w[COVIS_ROW_THREADS / 64];
  const int pos = blockIdx.y, s = (int)(blockIdx.x * COVIS_ROW_THREADS + threadIdx.x);
  const int p = lm_slot_point(a, pos, s);
  const bool win = p >= 0 && a.first[p] == lm::lm_key(pos, s);
  const uint64_t m = wave_ballot(win);
  const int w = wave_id();
  if (lane_id() == 0) s_w[w] = __popcll(m);
  __syncthreads();
  const int b = lm::lm_block(pos, blockIdx.x, a.nbx);
  if (b == 0 && threadIdx.x == 0) a.hdr[0] = a.blk[a.n_blocks];
  if (!win || b >= a.n_blocks) return;
  int off = a.blk[b];
  for (int k = 0; k < COVIS_ROW_THREADS / 64; k++) off += k < w ? s_w[k] : 0;
  const int idx = off + prefix_in_wave(m);
  if ((unsigned)idx >= (unsigned)a.bound) return;
  a.out[idx] = p;
  a.first[p] = lm::lm_tag(idx);  // equals no key: every other thread of p still loses
}

struct LmGatherArgs {
  const int32_t* hdr;    // hdr[0] = n_points
  int32_t* missing;      // hdr + 1
  const int32_t* out;    // [bound]
  int bound, P;
  const uint4* rec;      // [P * 4]
  const uint8_t* state;  // [P]
  uint4* desc;           // [bound * 2]
  uint32_t* pos;         // [bound * 3] float bits
  uint32_t* nrm;         // [bound * 3]
  uint32_t* min_d;       // [bound]
  uint32_t* max_d;       // [bound]
  uint8_t* flags;        // [bound]
};

// grid ceil(4 * bound / 256): lanes 4i .. 4i+3 move point i; 0, 1 the descriptor halves, 2, 3 the floats
__global__ __launch_bounds__(COVIS_ROW_THREADS) void k_lm_gather(LmGatherArgs g) {
  const long long t = (long long)blockIdx.x * COVIS_ROW_THREADS + threadIdx.x;
  const int i = (int)(t >> 2), q = (int)(t & 3);
  if (i >= g.bound || i >= g.hdr[0]) return;
  const int p = g.out[i];
  if ((unsigned)p >= (unsigned)g.P) return;
  const uint8_t st = g.state[p];
  if (!(st & lm::kPresent)) {
    if (q == 0) atomicAdd(g.missing, 1);
    return;
  }
  const uint4 v = g.rec[(size_t)p * 4 + q];
  if (q < 2) {
    g.desc[(size_t)i * 2 + q] = v;
    if (q == 0) g.flags[i] = (uint8_t)(st & ~lm::kPresent);
  } else if (q == 2) {
    g.pos[3 * (size_t)i] = v.x;
    g.pos[3 * (size_t)i + 1] = v.y;
    g.pos[3 * (size_t)i + 2] = v.z;
    g.nrm[3 * (size_t)i] = v.w;
  } else {
    g.nrm[3 * (size_t)i + 1] = v.x;
    g.nrm[3 * (size_t)i + 2] = v.y;
    g.min_d[i] = v.z;
    g.max_d[i] = v.w;
  }
}

// After the gather: the whole flag byte of a seen point is stored again with ORBFE_MPF_SEEN, so a point
// listed twice is written twice with the same value.
__global__ __launch_bounds__(COVIS_ROW_THREADS) void k_lm_seen(LmGatherArgs g, const uint32_t* first, int n_seen,
                                                               const int32_t* seen) {
  const int j = (int)(blockIdx.x * COVIS_ROW_THREADS + threadIdx.x);
  if (j >= n_seen) return;
  const int p = seen[j];
  if ((unsigned)p >= (unsigned)g.P) return;  // -1: no point
  const uint32_t v = first[p];
  if (!lm::lm_is_index(v)) return;  // bad, or in no named row
  const int idx = lm::lm_index(v);
  if (idx >= g.bound || idx >= g.hdr[0]) return;
  g.flags[idx] = (uint8_t)((g.state[p] & ~lm::kPresent) | ORBFE_MPF_SEEN);
}

__global__ __launch_bounds__(COVIS_ROW_THREADS) void k_lm_reset(LmArgs a) {
  const int i = (int)(blockIdx.x * COVIS_ROW_THREADS + threadIdx.x);
  if (i >= a.bound || i >= a.hdr[0]) return;
  const int p = a.out[i];
  if ((unsigned)p < (unsigned)a.P) a.first[p] = lm::kNone;
}

// grid ceil(4 * n / 256): the records of one staging pass into the store
__global__ __launch_bounds__(COVIS_ROW_THREADS) void k_lm_set_geometry(int n, const int32_t* ids, const uint8_t* flags,
                                                                       const uint4* src, int P, uint4* rec,
                                                                       uint8_t* state) {
  const long long t = (long long)blockIdx.x * COVIS_ROW_THREADS + threadIdx.x;
  const int i = (int)(t >> 2), q = (int)(t & 3);
  if (i >= n) return;
  const int p = ids[i];
  if ((unsigned)p >= (unsigned)P) return;
  rec[(size_t)p * 4 + q] = src[(size_t)i * 4 + q];
  if (q == 0) state[p] = (uint8_t)(flags[i] | lm::kPresent);
}

static const char* const kHostOnly = "covisibility table is host-only (device < 0)";

// The gathered SoA of `cap` points inside d_geo_out (cap a multiple of 64: every array 256-byte aligned).
static void covis_lm_geo_view(const orbfe_covis* h, LmGatherArgs* g) {
  const size_t cap = (size_t)h->geo_out_cap;
  uint8_t* b = h->d_geo_out;
  g->desc = reinterpret_cast<uint4*>(b);
  g->pos = reinterpret_cast<uint32_t*>(b + 32 * cap);
  g->nrm = reinterpret_cast<uint32_t*>(b + 44 * cap);
  g->min_d = reinterpret_cast<uint32_t*>(b + 56 * cap);
  g->max_d = reinterpret_cast<uint32_t*>(b + 60 * cap);
  g->flags = b + 64 * cap;
}

// The whole device pass for the list in h->tmp_rows. On return the stream is idle, h_res[0..1] hold
// n_points and n_missing, the ids are in d_res at word *ids_at.
static int covis_lm_run(orbfe_covis* h, const lm::Plan& plan, int n_kf, int n_seen, const int32_t* seen, bool gather,
                        int* n_points, int* n_missing, size_t* ids_at) {
  const cc::Core& c = h->core;
  *n_points = *n_missing = 0;
  *ids_at = 0;
  hipSetDevice(h->device);
  if (!h->d_lm_first) {
    ORBFE_HIP_CHECK(hipMalloc((void**)&h->d_lm_first, 4 * (size_t)c.P));
    h->lm_dirty = true;
  }
  if (h->lm_dirty) {
    ORBFE_HIP_CHECK(hipMemsetAsync(h->d_lm_first, 0xff, 4 * (size_t)c.P, h->stream));
    ORBFE_HIP_CHECK(hipStreamSynchronize(h->stream));
    h->lm_dirty = false;
  }
  if (plan.max_row == 0 || plan.bound == 0) return ORBFE_OK;  // every named row is empty
  int st = covis_stage_reserve(h, orbfe_al256(4 * (size_t)n_kf) + orbfe_al256(4 * (size_t)n_seen));
  if (st) return st;
  const size_t o_blk = 4, o_out = o_blk + (size_t)plan.n_blocks + 1, words = o_out + (size_t)plan.bound;
  st = covis_res_reserve(h, 4 * words);
  if (st) return st;
  if (gather && plan.bound > h->geo_out_cap) {
    ORBFE_HIP_CHECK(hipStreamSynchronize(h->stream));
    const long long want = std::max<long long>(plan.bound, (long long)h->geo_out_cap * 2);
    const int cap = (int)std::min<long long>((want + 63) & ~63ll, ((long long)c.P + 63) & ~63ll);
    hipFree(h->d_geo_out);
    h->d_geo_out = nullptr;
    h->geo_out_cap = 0;
    ORBFE_HIP_CHECK(hipMalloc((void**)&h->d_geo_out, 65 * (size_t)cap));
    h->geo_out_cap = cap;
  }
  const void *d_list, *d_seen = nullptr;
  st = covis_upload(h, h->tmp_rows.data(), 4 * (size_t)n_kf, nullptr, &d_list);
  if (st) return st;
  if (gather && n_seen > 0) {
    st = covis_upload(h, seen, 4 * (size_t)n_seen, nullptr, &d_seen);
    if (st) return st;
  }
  int32_t* d = reinterpret_cast<int32_t*>(h->d_res);
  LmArgs a;
  a.rows = h->d_rows;
  a.row_n = h->d_row_n;
  a.bad = h->d_bad;
  a.M = c.M;
  a.S = c.S;
  a.P = c.P;
  a.list_rows = (const int32_t*)d_list;
  a.n_kf = n_kf;
  a.nbx = plan.nbx;
  a.n_blocks = plan.n_blocks;
  a.first = h->d_lm_first;
  a.hdr = d;
  a.blk = d + o_blk;
  a.out = d + o_out;
  a.bound = plan.bound;
  const dim3 grid(plan.nbx, n_kf), block(COVIS_ROW_THREADS);
  const unsigned rb = (unsigned)((plan.bound + COVIS_ROW_THREADS - 1) / COVIS_ROW_THREADS);
  h->lm_dirty = true;  // until the reset below has run
  ORBFE_HIP_CHECK(hipMemsetAsync(d, 0, 16, h->stream));
  ORBFE_LAUNCH("k_lm_first", k_lm_first, grid, block, 0, h->stream, a);
  ORBFE_LAUNCH("k_lm_count", k_lm_count, grid, block, 0, h->stream, a);
  covis_scan(h, a.blk, plan.n_blocks);
  ORBFE_LAUNCH("k_lm_emit", k_lm_emit, grid, block, 0, h->stream, a);
  if (gather) {
    LmGatherArgs g;
    g.hdr = d;
    g.missing = d + 1;
    g.out = a.out;
    g.bound = plan.bound;
    g.P = c.P;
    g.rec = reinterpret_cast<const uint4*>(h->d_geo_rec);
    g.state = h->d_geo_state;
    covis_lm_geo_view(h, &g);
    const unsigned gb = (unsigned)((4ll * plan.bound + COVIS_ROW_THREADS - 1) / COVIS_ROW_THREADS);
    ORBFE_LAUNCH("k_lm_gather", k_lm_gather, dim3(gb), block, 0, h->stream, g);
    if (n_seen > 0)
      ORBFE_LAUNCH("k_lm_seen", k_lm_seen, dim3((n_seen + COVIS_ROW_THREADS - 1) / COVIS_ROW_THREADS), block, 0,
                   h->stream, g, (const uint32_t*)h->d_lm_first, n_seen, (const int32_t*)d_seen);
  }
  ORBFE_LAUNCH("k_lm_reset", k_lm_reset, dim3(rb), block, 0, h->stream, a);
  ORBFE_HIP_CHECK(hipGetLastError());
  ORBFE_HIP_CHECK(hipMemcpyAsync(h->h_res, d, 16, hipMemcpyDeviceToHost, h->stream));
  ORBFE_HIP_CHECK(hipStreamSynchronize(h->stream));
  h->lm_dirty = false;
  const int32_t* hres = reinterpret_cast<const int32_t*>(h->h_res);
  if (hres[0] < 0 || hres[0] > plan.bound || hres[1] < 0 || hres[1] > hres[0])
    return orbfe_set_error(ORBFE_ERR_STATE, "orbfe_covis_distinct_points: corrupt result");
  *n_points = hres[0];
  *n_missing = hres[1];
  *ids_at = o_out;
  return ORBFE_OK;
}

// n ids from word `at` of d_res to the caller
static int covis_lm_ids(orbfe_covis* h, size_t at, int n, int32_t* dst) {
  if (n == 0) return ORBFE_OK;
  ORBFE_HIP_CHECK(hipMemcpyAsync(h->h_res + 4 * at, h->d_res + 4 * at, 4 * (size_t)n, hipMemcpyDeviceToHost, h->stream));
  ORBFE_HIP_CHECK(hipStreamSynchronize(h->stream));
  memcpy(dst, h->h_res + 4 * at, 4 * (size_t)n);
  return ORBFE_OK;
}

extern "C" int orbfe_covis_distinct_points(orbfe_covis* h, int n_kf, const int64_t* kf_ids, orbfe_covis_points_t* r) {
  if (!h || !r || r->point_capacity < 0 || (r->point_capacity > 0 && !r->point_ids))
    return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_covis_distinct_points: bad argument");
  lm::Plan plan;
  cc::Status cs = lm::check_list(h->core, n_kf, kf_ids, &h->tmp_rows, &plan);
  if (cs) return covis_fail("orbfe_covis_distinct_points", cs);
  if (h->device < 0) return orbfe_set_error(ORBFE_ERR_STATE, kHostOnly);
  int np = 0, nm = 0;
  size_t at = 0;
  int st = covis_lm_run(h, plan, n_kf, 0, nullptr, false, &np, &nm, &at);
  if (st) return st;
  r->n_points = np;
  if (np > r->point_capacity)
    return orbfe_set_error(ORBFE_ERR_CAPACITY, "orbfe_covis_distinct_points: point_capacity below the result");
  return covis_lm_ids(h, at, np, r->point_ids);
}

extern "C" int orbfe_covis_set_point_geometry(orbfe_covis* h, int n, const int32_t* point_ids, const uint8_t* flags,
                                              const float* world_pos, const float* normal, const float* min_distance,
                                              const float* max_distance, const uint8_t* descriptors) {
  if (!h) return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_covis_set_point_geometry: bad argument");
  cc::Status cs = lm::check_geometry(h->core, n, point_ids, flags, world_pos, normal, min_distance, max_distance,
                                     descriptors);
  if (cs) return covis_fail("orbfe_covis_set_point_geometry", cs);
  if (h->device < 0 || n == 0) return ORBFE_OK;
  hipSetDevice(h->device);
  const size_t P = (size_t)h->core.P;
  if (!h->d_geo_rec) {
    uint8_t *rec = nullptr, *state = nullptr;
    ORBFE_HIP_CHECK(hipMalloc((void**)&rec, lm::kRecord * P));
    hipError_t e = hipMalloc((void**)&state, P);
    if (e == hipSuccess) e = hipMemsetAsync(state, 0, P, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
      hipFree(rec);
      hipFree(state);
      return orbfe_set_hip_error(e, "orbfe_covis_set_point_geometry: the store");
    }
    h->d_geo_rec = rec;
    h->d_geo_state = state;
  }
  for (int b = 0; b < n; b += lm::kSetChunk) {
    const int m = std::min(lm::kSetChunk, n - b);
    int st = covis_stage_reserve(h, orbfe_al256(lm::kRecord * (size_t)m) + orbfe_al256(4 * (size_t)m) + orbfe_al256((size_t)m));
    if (st) return st;
    const size_t off = covis_stage_take(h, lm::kRecord * (size_t)m);
    for (int i = 0; i < m; i++)
      lm::pack_record(h->h_stage + off + lm::kRecord * (size_t)i, b + i, world_pos, normal, min_distance, max_distance,
                      descriptors);
    ORBFE_HIP_CHECK(hipMemcpyAsync(h->d_stage + off, h->h_stage + off, lm::kRecord * (size_t)m, hipMemcpyHostToDevice,
                                   h->stream));
    const void *d_ids, *d_flags;
    st = covis_upload(h, point_ids + b, 4 * (size_t)m, nullptr, &d_ids);
    if (st) return st;
    st = covis_upload(h, flags + b, (size_t)m, nullptr, &d_flags);
    if (st) return st;
    ORBFE_LAUNCH("k_lm_set_geometry", k_lm_set_geometry,
                 dim3((unsigned)((4ll * m + COVIS_ROW_THREADS - 1) / COVIS_ROW_THREADS)), dim3(COVIS_ROW_THREADS), 0,
                 h->stream, m, (const int32_t*)d_ids, (const uint8_t*)d_flags,
                 reinterpret_cast<const uint4*>(h->d_stage + off), h->core.P, reinterpret_cast<uint4*>(h->d_geo_rec),
                 h->d_geo_state);
    ORBFE_HIP_CHECK(hipGetLastError());
    ORBFE_HIP_CHECK(hipStreamSynchronize(h->stream));  // the next pass reuses the staging
  }
  return ORBFE_OK;
}

extern "C" int orbfe_covis_local_geometry(orbfe_covis* h, int n_kf, const int64_t* kf_ids, int n_seen,
                                          const int32_t* seen_point_ids, orbfe_covis_local_geometry_t* r) {
  if (!h || !r || r->point_capacity < 0 || (r->point_capacity > 0 && !r->point_ids))
    return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_covis_local_geometry: bad argument");
  lm::Plan plan;
  cc::Status cs = lm::check_list(h->core, n_kf, kf_ids, &h->tmp_rows, &plan);
  if (cs) return covis_fail("orbfe_covis_local_geometry", cs);
  cs = lm::check_seen(h->core, n_seen, seen_point_ids);
  if (cs) return covis_fail("orbfe_covis_local_geometry", cs);
  if (h->device < 0) return orbfe_set_error(ORBFE_ERR_STATE, kHostOnly);
  r->n_points = r->n_missing = 0;
  memset(&r->geometry, 0, sizeof(r->geometry));
  int np = 0, nm = 0;
  size_t at = 0;
  int st;
  if (!h->d_geo_rec) {  // an empty store: every point of the list is missing
    st = covis_lm_run(h, plan, n_kf, 0, nullptr, false, &np, &nm, &at);
    nm = np;
  } else {
    st = covis_lm_run(h, plan, n_kf, n_seen, seen_point_ids, true, &np, &nm, &at);
  }
  if (st) return st;
  r->n_points = np;
  r->n_missing = nm;
  if (np > r->point_capacity)
    return orbfe_set_error(ORBFE_ERR_CAPACITY, "orbfe_covis_local_geometry: point_capacity below the result");
  st = covis_lm_ids(h, at, np, r->point_ids);
  if (st) return st;
  if (nm > 0) return orbfe_set_error(ORBFE_ERR_STATE, "orbfe_covis_local_geometry: a point's geometry was never set");
  if (np == 0) return ORBFE_OK;
  LmGatherArgs g;
  covis_lm_geo_view(h, &g);
  r->geometry.m = np;
  r->geometry.flags = g.flags;
  r->geometry.world_pos = reinterpret_cast<const float*>(g.pos);
  r->geometry.normal = reinterpret_cast<const float*>(g.nrm);
  r->geometry.min_distance = reinterpret_cast<const float*>(g.min_d);
  r->geometry.max_distance = reinterpret_cast<const float*>(g.max_d);
  r->geometry.descriptors = reinterpret_cast<const uint8_t*>(g.desc);
  return ORBFE_OK;
}

// ------------------------------------------------------------------------------------------
// orbfe_covis_view.h: the rows and the geometry store as orbfe_gridmap.hip reads them. Every mutation
// above synchronises the handle's stream before it returns, so the arrays are complete here.
int orbfe_covis_rows_view(orbfe_covis* h, int n_kf, const int64_t* kf_ids, std::vector<int32_t>* list_rows,
                          std::vector<int32_t>* row_len, CovisRowsView* view) {
  if (!h || !list_rows || !row_len || !view) return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_covis_rows_view: bad argument");
  lm::Plan plan;
  cc::Status cs = lm::check_list(h->core, n_kf, kf_ids, list_rows, &plan);
  if (cs) return covis_fail("orbfe_gridmap_update_resident", cs);
  row_len->resize(n_kf);
  for (int i = 0; i < n_kf; i++) (*row_len)[i] = std::min(std::max(h->core.row_n[(*list_rows)[i]], 0), h->core.S);
  view->device = h->device;
  view->rows = h->d_rows;
  view->row_n = h->d_row_n;
  view->bad = h->d_bad;
  view->geo_rec = h->d_geo_rec;
  view->geo_state = h->d_geo_state;
  view->M = h->core.M;
  view->S = h->core.S;
  view->P = h->core.P;
  return ORBFE_OK;
}
