/*
 * orbfe_essgraph.h -- Optimizer::OptimizeEssentialGraph on the GPU (liborbfe.so, gfx950): the pose-graph
 * Levenberg-Marquardt over Sim3 vertices that LoopClosing::CorrectLoop runs after a loop is accepted,
 * solved by a sparse LDL^T over the block envelope of the Hessian.
 *
 * Replaces, in the reference (lreithmayr/ORB_SLAM2_2021):
 *   Optimizer::OptimizeEssentialGraph, from the optimizer's set-up on   src/Optimizer.cc:784-1048
 *   Converter::toMatrix3d / toVector3d / toCvSE3 / toCvMat              src/Converter.cc
 * and what it runs of g2o: Sim3 (the constructors, operator*, inverse, map, log), VertexSim3Expmap
 * (oplusImpl), EdgeSim3 (computeError), BaseBinaryEdge (the numeric linearizeOplus,
 * constructQuadraticForm), BlockSolver_7_3 (buildSystem, setLambda, restoreDiagonal, the non-Schur
 * solve), OptimizationAlgorithmLevenberg (solve, setUserLambdaInit, computeScale) and SparseOptimizer
 * (initializeOptimization, optimize, push, pop, discardTop, update, activeRobustChi2).
 *
 * The caller performs the gather of Optimizer.cc:800-988: the non-bad
 * keyframes ascending in mnId with GetRotation() / GetTranslation(), the index of pLoopKF, the entries of
 * CorrectedSim3 and NonCorrectedSim3 as (vertex index, q x y z w, t, s), the edges as (vertex 0, vertex 1,
 * kind) -- kind 0 a loop-connection edge (:853-885, measured over vScw), kind 1 a spanning-tree, loop or
 * covisibility edge (:887-988, measured over NonCorrectedSim3 where the keyframe is in it) -- and the map
 * points with the vertex index :1025-1034 choose. The measurements are computed on the device, in double.
 *
 * Carried as written: EdgeSim3's error (C * v0 * v1^-1).log() with log()'s four branches and its 3x3
 * partial-pivot LU; the identity information, no robust kernel; numeric Jacobians (+-1e-9, times
 * 1 / 2e-9) per free vertex, none for the fixed vertex; with fix_scale column 6 is +0 and H66 = lambda;
 * lambda starts at 1e-16 (setUserLambdaInit); optimize(20) with the rho test, qmax and _nBad of
 * OptimizationAlgorithmLevenberg; a vertex without an edge keeps its estimate; every vertex, the fixed
 * one included, is written out as [R | t / s]; a point is mapped by vScw[ref] (the start estimate) and
 * the optimised inverse.
 *
 * Deviations, deliberate:
 *  - fixed summation order (g2o's follows pointer-ordered containers): a vertex's H_ii and b_i run over
 *    its edges in ascending edge index from +0.0, an off-diagonal block over its edges likewise; for the
 *    total chi2 edge e, and for computeScale free vertex s, belongs to lane index % 64, a lane adds in
 *    ascending index from +0.0, the lanes are combined by s[l] += s[l + stride], stride = 32 .. 1.
 *  - the linear solve is an unpivoted LDL^T in natural (caller) order over the block envelope (the
 *    reference: Eigen's SimplicialLDLT with AMD ordering): the free vertices that have an edge are
 *    renumbered in order, row i stores the 7x7 blocks from its first structurally non-zero block column
 *    to the diagonal, all fill falls inside. Per scalar: v = A_ij, v -= (L_ik d_k) L_jk for k ascending,
 *    L_ij = v / d_j. A trial fails when a d_j is 0.
 *  - ORBFE_ESSGRAPH_FLAG_NONFINITE: a non-finite d_j fails the trial.
 *  - exp, sin, cos and pow(., 3) as in orbfe_optsim3.h (ORBFE_ESSGRAPH_FLAG_LARGE_STEP); log and acos
 *    from + - * / sqrt after fdlibm (within 2 ulp of libm); Eigen's small fixed-size products in plain
 *    left-to-right order; the information matrix read as the identity it is.
 *  - x is zero before the first successful solve and keeps the last successful solve's value after a
 *    failed one.
 *  - CorrectedSim3 / NonCorrectedSim3 entries are taken as given (q not normalised, as Sim3 never does).
 *
 * Bounds: 8,192 vertices, 65,536 edges, 524,288 envelope blocks, 1,048,576 map points (a workspace of
 * about 0.6 GiB at the caps). A handle is not thread-safe.
 */
#ifndef ORBFE_ESSGRAPH_H
#define ORBFE_ESSGRAPH_H
#include <stdint.h>

#include "orbfe.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct orbfe_essgraph orbfe_essgraph;

#define ORBFE_ESSGRAPH_MAX_VERTICES 8192
#define ORBFE_ESSGRAPH_MAX_EDGES 65536
#define ORBFE_ESSGRAPH_MAX_ENV_BLOCKS 524288 /* 7x7 doubles each, held twice */
#define ORBFE_ESSGRAPH_MAX_POINTS 1048576

#define ORBFE_ESSGRAPH_FLAG_LARGE_STEP 1u
#define ORBFE_ESSGRAPH_FLAG_NONFINITE 2u

/* why optimize() ended */
#define ORBFE_ESSGRAPH_STOP_ALL 0        /* ran all 20 iterations */
#define ORBFE_ESSGRAPH_STOP_TERMINATE 1  /* 10 trials in one iteration, or rho == 0 */
#define ORBFE_ESSGRAPH_STOP_NBAD 2       /* three iterations in a row gained less than 1e-3 of their chi2 */
#define ORBFE_ESSGRAPH_STOP_NO_EDGE 3    /* no edge: optimize() returned without a step */

/* device < 0: a host-only handle (argument checks work, a solve that gets past them returns
 * ORBFE_ERR_STATE). ORBFE_ERR_ARG past the hard caps above. max_points may be 0. */
int orbfe_essgraph_create(int device, int max_vertices, int max_edges, int max_env_blocks, int max_points,
                          orbfe_essgraph** out);
int orbfe_essgraph_destroy(orbfe_essgraph* h);

typedef struct {
  int n_vertices;
  const float* tcw;              /* [n_vertices*12] [GetRotation() | GetTranslation()], row-major 3x4 */
  int fixed_vertex;              /* pLoopKF */
  int fix_scale;                 /* bFixScale */
  int n_corrected;
  const int* corrected_idx;      /* [n_corrected] */
  const double* corrected_sim3;  /* [n_corrected*8] q x y z w, t, s */
  int n_noncorrected;
  const int* noncorrected_idx;
  const double* noncorrected_sim3;
  int n_edges;
  const int* edge_i;             /* [n_edges] vertex 0 */
  const int* edge_j;             /* [n_edges] vertex 1 */
  const uint8_t* edge_kind;      /* [n_edges] 0: loop connection, 1: spanning tree / loop / covisibility */
  int n_points;                  /* may be 0 */
  const float* xw;               /* [n_points*3] GetWorldPos() */
  const int* point_ref;          /* [n_points] mnCorrectedReference or the reference keyframe */
} orbfe_essgraph_problem_t;

typedef struct {
  int iterations;       /* solve() calls */
  int trials;           /* Levenberg trials over all iterations */
  int rejected_trials;
  int stop;             /* ORBFE_ESSGRAPH_STOP_* */
  double lambda;        /* _currentLambda at the end */
  double chi2;          /* the last currentChi */
  int env_blocks;       /* 7x7 blocks of the envelope */
  uint32_t flags;       /* ORBFE_ESSGRAPH_FLAG_* */
} orbfe_essgraph_trace_t;

typedef struct {
  float* tcw;  /* out [n_vertices*12]: what SetPose receives, [R | t / s] */
  float* xw;   /* out [n_points*3]: what SetWorldPos receives */
  orbfe_essgraph_trace_t trace;
} orbfe_essgraph_result_t;

/* ORBFE_ERR_CAPACITY past the handle's bounds (vertices, edges, points, envelope blocks);
 * ORBFE_ERR_ARG for a null array, an index out of range, an edge with i == j, a kind above 1 or a
 * keyframe listed twice in one of the two maps. The Levenberg control flow runs on the host: one small
 * record is read back per linearisation and per trial; every kernel is launched on the handle's one
 * stream. */
int orbfe_essgraph_solve(orbfe_essgraph* h, const orbfe_essgraph_problem_t* problem, orbfe_essgraph_result_t* result);

#ifdef __cplusplus
}
#endif
#endif
