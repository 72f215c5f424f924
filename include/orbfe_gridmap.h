/*
 * orbfe_gridmap.h -- the 2-D occupancy grid of the reference's fourth thread on the GPU
 * (liborbfe.so, gfx950): one Bresenham "laser beam" per map point of a keyframe into a visit
 * counter, one increment per point into an occupied counter, and the int8 grid message built from
 * the two.
 *
 * Replaces, in the reference (lreithmayr/ORB_SLAM2_2021):
 *   GridMapping::InitGridMap            src/GridMapping.cpp:72-107
 *   GridMapping::UpdateGridMap          src/GridMapping.cpp:109-135
 *   GridMapping::BuildOccupancyGridMsg  src/GridMapping.cpp:137-154
 *   GridMapping::ResetGridMap           src/GridMapping.cpp:176-181
 *   GridMapping::CastLaserBeam          src/GridMapping.cpp:232-270
 * ROS publishing, the pose message, PublishPC and the derivation of Ow from Tcw stay with the caller.
 *
 * Every rule is restated in orb_slam2_2021_amd/csrc/orbfe_gridmap_core.h and used by both the kernels
 * and the _host functions; DESIGN.md §29 records the rules and the decisions. Counters and the grid
 * are integers and exact: increments commute, so a result does not depend on the order of execution,
 * and the device and the host entry points agree bit for bit.
 *
 * Geometry. cols = max_x - min_x and rows = max_z - min_z (float differences) must be integral and
 * >= 1 (else ORBFE_ERR_ARG) with rows * cols < 2^31 (else ORBFE_ERR_CAPACITY); scale_factor >= 1 and
 * visit_threshold >= 0 (else ORBFE_ERR_ARG: with a negative threshold an unvisited cell divides 0 by
 * 0). norm = float(size - 1) / float(size). Counters are int32, row-major [rows][cols].
 *
 * The cell of a position, in float: g = p * (float)scale_factor, c = (g - min) * norm, floor, int;
 * outside when < 0 or >= size. A NaN, or a floored value outside the int range, is outside.
 *
 * Rules.
 *   ORBFE_GRIDMAP_REFERENCE: what the reference's code does. CastLaserBeam takes its ends by
 *     reference, so its swaps rewrite the keyframe's cell: beam i of a keyframe starts at the state
 *     the swaps of beams 0..i-1 left behind (possibly transposed, possibly an earlier point's cell);
 *     and the first point outside the grid ends the keyframe (its remaining points are dropped).
 *     A visit goes to the flat index row * cols + col that the reference's unchecked at<int>()
 *     addresses, so col >= cols lands in a later row; a flat index >= rows * cols is dropped and
 *     counted (the reference writes past its buffer there).
 *   ORBFE_GRIDMAP_INTENDED: what include/GridMapping.h documents. Every beam starts at the
 *     keyframe's cell; a point outside the grid is skipped and the rest still count.
 * In both, a keyframe whose own cell is outside the grid contributes nothing.
 *
 * The message: data = vc <= visit_threshold ? 1 : 1 - float(oc) / float(vc);
 * msg = (1 - data) * 100 truncated to int, then clamped to [-128, 127] (identical wherever the
 * reference's float -> int8_t conversion is defined). Only the int8 grid is stored; the float grid
 * of a row range is produced on request.
 *
 * Bounds: n_kf 1..4096 keyframes per call, 0..8192 points per keyframe. Device scratch per handle,
 * allocated at create: 32 bytes for each of 2^18 points (a call is worked off in groups of whole
 * keyframes of at most that many points), 20 bytes for each of max(2^22, ceil(max(rows, cols) / 64))
 * beam segments, and a 16 MiB staging buffer for orbfe_gridmap_probability: 104 MiB for the default
 * geometry, beside the 9 bytes per cell of the counters and the grid. A handle is not thread-safe.
 */
#ifndef ORBFE_GRIDMAP_H
#define ORBFE_GRIDMAP_H
#include <stdint.h>

#include "orbfe.h"
#include "orbfe_covis.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct orbfe_gridmap orbfe_gridmap;

#define ORBFE_GRIDMAP_REFERENCE 0
#define ORBFE_GRIDMAP_INTENDED 1

/* Steps of a beam per work item of the scatter pass (one step = one visited cell). */
#define ORBFE_GRIDMAP_SEGMENT 64
#define ORBFE_GRIDMAP_MAX_KEYFRAMES 4096
#define ORBFE_GRIDMAP_MAX_POINTS 8192

typedef struct orbfe_gridmap_geometry {
  int32_t scale_factor;
  float min_x, max_x, min_z, max_z;
  int32_t visit_threshold;
} orbfe_gridmap_geometry;

/* The reference's values: scale 3, x in -3000..3000, z in -1500..4800 (6300 rows x 6000 cols),
 * visit_threshold 0. */
int orbfe_gridmap_default_geometry(orbfe_gridmap_geometry* g);
/* rows, cols and the two norm factors of a geometry, after the checks above. Host only. */
int orbfe_gridmap_dims(const orbfe_gridmap_geometry* g, int32_t* rows, int32_t* cols, float* norm_x,
                       float* norm_z);

/* What one update did. visits counts the increments applied, dropped those whose flat index lay
 * beyond the grid. points_cut: under REFERENCE rules the points from a keyframe's first outside
 * point to its last, under INTENDED rules the outside points skipped (points of a keyframe that is
 * itself outside are not counted). [row0, row1): the rows an increment of either counter touched --
 * from a handle, accumulated since the last build (row0 == row1: none); from
 * orbfe_gridmap_host_update, of that call alone. */
typedef struct orbfe_gridmap_stats {
  int64_t beams;
  int64_t visits;
  int64_t dropped;
  int64_t points_cut;
  int32_t kf_outside;
  int32_t row0, row1;
} orbfe_gridmap_stats;

/* device < 0: a host-only handle (the argument checks work, every call that needs the device returns
 * ORBFE_ERR_STATE after them). Both counters and the grid start at zero. */
int orbfe_gridmap_create(int device, const orbfe_gridmap_geometry* g, int rules, orbfe_gridmap** out);
int orbfe_gridmap_destroy(orbfe_gridmap* h);
/* ResetGridMap: both counters to zero; the grid becomes the message of an empty map (all zero) and
 * the dirty range is cleared. */
int orbfe_gridmap_reset(orbfe_gridmap* h);

/* UpdateGridMap of n_kf keyframes in one call: centres[n_kf * 3] (the caller's Ow: x, y, z) and a CSR
 * of world positions in GetMPs order (KeyFrame.cc:251-263): keyframe k owns points
 * begin[k] .. begin[k + 1] of world_pos[begin[n_kf] * 3]; begin[0] == 0. The loop-closure rebuild is
 * reset followed by one update over every keyframe. n_kf > 4096 or a keyframe of more than 8192
 * points: ORBFE_ERR_CAPACITY; n_kf < 1, a NULL array or a descending begin: ORBFE_ERR_ARG; all
 * before any device work. Blocking; stats may be NULL. */
int orbfe_gridmap_update(orbfe_gridmap* h, int n_kf, const float* centres, const int32_t* begin,
                         const float* world_pos, orbfe_gridmap_stats* stats);

/* The same update over the rows of an orbfe_covis handle on the same device: the points of keyframe
 * kf_ids[k] are its row's slots in slot order, slots holding -1 or a point flagged bad skipped; their
 * positions are the world_pos of the geometry store (orbfe_localmap.h). An id that is not stored:
 * ORBFE_ERR_ARG. A point whose geometry was never set: ORBFE_ERR_STATE with *n_missing = how many
 * (slots, counted on the device before anything else runs); no counter is touched then.
 * n_missing may be NULL. */
int orbfe_gridmap_update_resident(orbfe_gridmap* h, orbfe_covis* covis, int n_kf, const int64_t* kf_ids,
                                  const float* centres, orbfe_gridmap_stats* stats, int32_t* n_missing);

/* BuildOccupancyGridMsg over the dirty rows (all_rows == 0) or over every row; clears the dirty
 * range. Rows outside the dirty range already hold the message of their counters. */
int orbfe_gridmap_build(orbfe_gridmap* h, int all_rows);

/* Rows [row0, row1) of the int8 grid / of both counters / of the float data grid to host arrays of
 * (row1 - row0) * cols entries; 0 <= row0 <= row1 <= rows, else ORBFE_ERR_ARG. upload_counters
 * overwrites the rows and marks them dirty. Either counter pointer may be NULL (skipped). Blocking. */
int orbfe_gridmap_download(orbfe_gridmap* h, int row0, int row1, int8_t* grid);
int orbfe_gridmap_download_counters(orbfe_gridmap* h, int row0, int row1, int32_t* occupied, int32_t* visits);
int orbfe_gridmap_upload_counters(orbfe_gridmap* h, int row0, int row1, const int32_t* occupied,
                                  const int32_t* visits);
int orbfe_gridmap_probability(orbfe_gridmap* h, int row0, int row1, float* data);

/* The same rules on host arrays (no device, no handle): occupied and visits hold rows * cols entries
 * and are incremented in place; grid (and data, unless NULL) receive rows [row0, row1) at
 * (row - row0) * cols. */
int orbfe_gridmap_host_update(const orbfe_gridmap_geometry* g, int rules, int32_t* occupied, int32_t* visits,
                              int n_kf, const float* centres, const int32_t* begin, const float* world_pos,
                              orbfe_gridmap_stats* stats);
int orbfe_gridmap_host_build(const orbfe_gridmap_geometry* g, const int32_t* occupied, const int32_t* visits,
                             int row0, int row1, int8_t* grid, float* data);

#ifdef __cplusplus
}
#endif
#endif
