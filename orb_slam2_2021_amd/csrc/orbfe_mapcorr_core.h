// orbfe_mapcorr_core.h -- the arithmetic of the three map corrections (include/orbfe_mapcorr.h):
// MapPoint::UpdateNormalAndDepth (MapPoint.cc:360-401), LoopClosing::CorrectLoop's pose and point
// correction (LoopClosing.cc:453-535) and RunGlobalBundleAdjustment's map update (:705-766), as
// host/device inline functions over one item each (a point, a keyframe, a row slot), and the serial
// compositions of them on the host (mc_host_*). Used by the kernels of orbfe_mapcorr.hip and by the
// stand-alone host program tests/cpp/mapcorr_core_test.cpp. Not part of the C ABI.
//
// Every operation is an IEEE float or double + - * / sqrt, rounded separately (-ffp-contract=off). The
// Sim3 and quaternion rules are orbfe_optsim3_core.h's and orbfe_poseopt_core.h's ("EIGEN:" there); a rule
// recalled from OpenCV's source carries "OPENCV:" (DESIGN.md sections 15 and 16). tests/mapcorr_ref.py is
// the same code in Python, line by line.
//
// Every index an item reads was checked by the caller (orbfe_mapcorr.hip's checks, the test program's
// readers); every loop runs to a count among those.
#pragma once
#include <vector>

#include "orbfe_optsim3_core.h"  // OsSim3, os_sim3_*, the quaternion rules

#define MC_NONE 0x7f7f7f7f  // corrected_by before the marks: above every list position (memset bytes 0x7f)

// OPENCV: CV_32F gemm element / cv::norm's sum of three float pairs: double accumulation left to right
PO_HD inline double mc_dot3(float a0, float a1, float a2, float b0, float b1, float b2) {
  double s = (double)a0 * (double)b0;
  s = s + (double)a1 * (double)b1;
  s = s + (double)a2 * (double)b2;
  return s;
}

// KeyFrame::SetPose: Ow = -Rwc * tcw, Rwc = Rcw^T. T: rows 0..2 of a pose, row-major.
// OPENCV: one gemm with alpha = -1: the double sum times alpha in double, one rounding
PO_HD inline void mc_centre(const float* T, float* ow) {
  ow[0] = (float)(-1.0 * mc_dot3(T[0], T[4], T[8], T[3], T[7], T[11]));
  ow[1] = (float)(-1.0 * mc_dot3(T[1], T[5], T[9], T[3], T[7], T[11]));
  ow[2] = (float)(-1.0 * mc_dot3(T[2], T[6], T[10], T[3], T[7], T[11]));
}

// KeyFrame::SetPose's Twc = [Rcw^T | Ow] (rows 0..2; the fourth row is [0 0 0 1])
PO_HD inline void mc_pose_inverse(const float* T, float* twc) {
  float ow[3];
  mc_centre(T, ow);
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) twc[4 * r + c] = T[4 * c + r];
    twc[4 * r + 3] = ow[r];
  }
}

// Rows 0..2 of the 4x4 product A * B of two poses whose fourth rows are [0 0 0 1].
// OPENCV: CV_32F gemm: each element the four-term double sum, k ascending, one rounding
PO_HD inline void mc_gemm44(const float* A, const float* B, float* out) {
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 4; c++) {
      const float b3 = c == 3 ? 1.0f : 0.0f;
      double s = (double)A[4 * r] * (double)B[c];
      s = s + (double)A[4 * r + 1] * (double)B[4 + c];
      s = s + (double)A[4 * r + 2] * (double)B[8 + c];
      s = s + (double)A[4 * r + 3] * (double)b3;
      out[4 * r + c] = (float)s;
    }
}

PO_HD inline void mc_load(const double* s, OsSim3* S) {
  for (int k = 0; k < 4; k++) S->q[k] = s[k];
  for (int k = 0; k < 3; k++) S->t[k] = s[4 + k];
  S->s = s[7];
}

// Sim3(toMatrix3d(R), toVector3d(t), 1.0) of a pose's widened floats
PO_HD inline void mc_sim3_of_pose(const float* T, OsSim3* S) {
  const float r9[9] = {T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10]};
  const float t3[3] = {T[3], T[7], T[11]};
  os_sim3_from_floats(r9, t3, 1.0, S);
}

// Sim3::map: s * (r * xyz) + t
PO_HD inline void mc_sim3_map(const OsSim3& S, const double* X, double* o) {
  double r[3];
  po_quat_rotate(S.q, X, r);
  for (int k = 0; k < 3; k++) o[k] = S.s * r[k] + S.t[k];
}

// ---- MapPoint::UpdateNormalAndDepth -------------------------------------------------------------------
struct McNd {
  const float* ow;        // [n_kf*3] GetCameraCenter() of every keyframe
  const float* ow_new;    // correct_loop: [n_connected*3] the centres of tcw_out by list position; else null
  const int* pos_of_kf;   // correct_loop: [n_kf] the list position of a connected keyframe, -1 otherwise; else null
  const float* scale;     // [n_levels] mvScaleFactors
  int n_levels;
  const int* obs_begin;   // [n_points+1]
  const int* obs_kf;
  const int* ref_kf;      // [n_points]
  const int* ref_level;   // [n_points]
  float* normal;          // [n_points*3]
  float* max_dist;        // [n_points]
  float* min_dist;        // [n_points]
  uint8_t* updated;       // [n_points]
};

// The camera centre keyframe k shows while the loop of list position r runs (LoopClosing.cc:519 comes
// before position r's SetPose): the new one only for a connected keyframe at a position below r
PO_HD inline const float* mc_nd_centre(const McNd& w, int k, int r) {
  if (w.pos_of_kf) {
    const int pos = w.pos_of_kf[k];
    if (pos >= 0 && pos < r) return w.ow_new + 3 * (size_t)pos;
  }
  return w.ow + 3 * (size_t)k;
}

// MapPoint.cc:375-400 for a point that is not bad, at the position X
PO_HD inline void mc_update_normal_depth(const McNd& w, int p, const float* X, int r) {
  const int b = w.obs_begin[p], e = w.obs_begin[p + 1];
  if (e <= b) {  // observations.empty()
    w.updated[p] = 0;
    return;
  }
  float n0 = 0.0f, n1 = 0.0f, n2 = 0.0f;  // cv::Mat::zeros(3, 1, CV_32F)
  for (int i = b; i < e; i++) {
    const float* O = mc_nd_centre(w, w.obs_kf[i], r);
    const float d0 = X[0] - O[0], d1 = X[1] - O[1], d2 = X[2] - O[2];
    const double nrm = sqrt(mc_dot3(d0, d1, d2, d0, d1, d2));  // OPENCV: cv::norm of CV_32F: the squares accumulate in double
    const float a = (float)(1.0 / nrm);                         // OPENCV: Mat / scalar multiplies by (float)(1.0 / s)
    n0 = n0 + d0 * a;
    n1 = n1 + d1 * a;
    n2 = n2 + d2 * a;
  }
  const float* O = mc_nd_centre(w, w.ref_kf[p], r);
  const float c0 = X[0] - O[0], c1 = X[1] - O[1], c2 = X[2] - O[2];
  const float dist = (float)sqrt(mc_dot3(c0, c1, c2, c0, c1, c2));  // const float dist = cv::norm(PC)
  const float maxd = dist * w.scale[w.ref_level[p]];
  const float inv = (float)(1.0 / (double)(e - b));  // OPENCV: normal / n multiplies by (float)(1.0 / n)
  w.max_dist[p] = maxd;
  w.min_dist[p] = maxd / w.scale[w.n_levels - 1];
  w.normal[3 * (size_t)p] = n0 * inv;
  w.normal[3 * (size_t)p + 1] = n1 * inv;
  w.normal[3 * (size_t)p + 2] = n2 * inv;
  w.updated[p] = 1;
}

// call 1: one point
PO_HD inline void mc_nd_point(const McNd& w, const float* xw, const uint8_t* bad, int p) {
  if (bad[p]) {  // if (mbBad) return
    w.updated[p] = 0;
    return;
  }
  mc_update_normal_depth(w, p, xw + 3 * (size_t)p, 0);
}

// ---- LoopClosing::CorrectLoop, :453-535 ---------------------------------------------------------------
struct McLoop {
  McNd nd;  // nd.ow: the old centres of all keyframes; nd.ow_new and nd.pos_of_kf set
  int n_kf, n_connected, cur, n_points, n_slots;
  const float* tcw;          // [n_kf*12]
  const int* connected_kf;   // [n_connected]
  double scw[8];
  const int* row_begin;      // [n_connected+1]
  const int* row_point;      // [n_slots]
  const float* xw;           // [n_points*3]
  const uint8_t* bad;        // [n_points]
  float* ow_old;             // [n_kf*3]        == nd.ow
  float* ow_new;             // [n_connected*3] == nd.ow_new
  double* nonc;              // [n_connected*8] NonCorrectedSim3
  double* corr;              // [n_connected*8] CorrectedSim3
  double* swi;               // [n_connected*8] its inverses
  float* tcw_out;            // [n_connected*12]
  float* xw_out;             // [n_points*3]
  int* corrected_by;         // [n_points] MC_NONE before the marks
};

// :465-488 and :522-531 for the keyframe at list position i
PO_HD inline void mc_loop_kf(const McLoop& w, int i) {
  const float* Tiw = w.tcw + 12 * (size_t)w.connected_kf[i];
  OsSim3 Scw, C, N, inv;
  mc_load(w.scw, &Scw);
  if (i != w.cur) {
    float Twc[12], Tic[12];
    mc_pose_inverse(w.tcw + 12 * (size_t)w.connected_kf[w.cur], Twc);  // mpCurrentKF->GetPoseInverse()
    mc_gemm44(Tiw, Twc, Tic);                                          // Tic = Tiw * Twc
    OsSim3 Sic;
    mc_sim3_of_pose(Tic, &Sic);
    os_sim3_mul(Sic, Scw, &C);  // g2oCorrectedSiw = g2oSic * mg2oScw
  } else {
    C = Scw;  // CorrectedSim3[mpCurrentKF] = mg2oScw
  }
  mc_sim3_of_pose(Tiw, &N);
  os_sim3_inverse(C, &inv);
  os_store_state(w.nonc + 8 * (size_t)i, N);
  os_store_state(w.corr + 8 * (size_t)i, C);
  os_store_state(w.swi + 8 * (size_t)i, inv);
  double m[9];
  po_quat_to_matrix(C.q, m);  // rotation().toRotationMatrix(): no normalisation
  const double c = 1. / C.s;  // eigt *= (1. / s)
  float* o = w.tcw_out + 12 * (size_t)i;
  for (int r = 0; r < 3; r++) {
    for (int k = 0; k < 3; k++) o[4 * r + k] = (float)m[3 * r + k];
    o[4 * r + 3] = (float)(C.t[r] * c);
  }
  mc_centre(o, w.ow_new + 3 * (size_t)i);
}

// Row slot t: its point is held by the row's list position. The first position wins (:507).
PO_HD inline void mc_loop_mark(const McLoop& w, int t) {
  const int p = w.row_point[t];
  if (p < 0 || w.bad[p]) return;
  int lo = 0, hi = w.n_connected;  // the last position whose row begins at or before t
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (w.row_begin[mid] <= t) lo = mid;
    else hi = mid;
  }
#if defined(__HIP_DEVICE_COMPILE__)
  atomicMin(w.corrected_by + p, lo);
#else
  if (lo < w.corrected_by[p]) w.corrected_by[p] = lo;
#endif
}

// :510-519 for point p
PO_HD inline void mc_loop_point(const McLoop& w, int p) {
  const int r = w.corrected_by[p];
  const float* x = w.xw + 3 * (size_t)p;
  float* o = w.xw_out + 3 * (size_t)p;
  if (r == MC_NONE) {
    w.corrected_by[p] = -1;
    o[0] = x[0], o[1] = x[1], o[2] = x[2];
    w.nd.updated[p] = 0;
    return;
  }
  OsSim3 Siw, Swi;
  mc_load(w.nonc + 8 * (size_t)r, &Siw);
  mc_load(w.swi + 8 * (size_t)r, &Swi);
  const double X[3] = {(double)x[0], (double)x[1], (double)x[2]};
  double a[3], c[3];
  mc_sim3_map(Siw, X, a);  // g2oCorrectedSwi.map(g2oSiw.map(eigP3Dw))
  mc_sim3_map(Swi, a, c);
  o[0] = (float)c[0], o[1] = (float)c[1], o[2] = (float)c[2];
  mc_update_normal_depth(w.nd, p, o, r);
}

// ---- LoopClosing::RunGlobalBundleAdjustment, :705-766 -------------------------------------------------
struct McGba {
  int n_kf, n_points;
  const float* tcw;          // [n_kf*12] GetPose(): mTcwBefGBA
  const float* tcw_gba;      // [n_kf*12]
  const uint8_t* optimised;  // [n_kf]
  const int* parent;         // [n_kf]
  const int* order;          // [n_kf] the keyframes by their distance to the nearest optimised ancestor
  const float* xw;
  const uint8_t* bad;
  const uint8_t* pt_optimised;
  const float* xw_gba;
  const int* ref_kf;
  float* tcw_out;            // [n_kf*12] mTcwGBA after the propagation: what SetPose receives
  float* ow_out;             // [n_kf*3] its camera centres
  float* xw_out;
  uint8_t* pt_changed;
};

// :716-727 for keyframe k; its parent's tcw_out is complete
PO_HD inline void mc_gba_kf(const McGba& w, int k) {
  float* o = w.tcw_out + 12 * (size_t)k;
  if (w.optimised[k]) {
    for (int i = 0; i < 12; i++) o[i] = w.tcw_gba[12 * (size_t)k + i];
  } else {
    const int q = w.parent[k];
    float Twc[12], Tchildc[12];
    mc_pose_inverse(w.tcw + 12 * (size_t)q, Twc);         // pKF->GetPoseInverse(): the parent's old pose
    mc_gemm44(w.tcw + 12 * (size_t)k, Twc, Tchildc);      // pChild->GetPose() * Twc
    mc_gemm44(Tchildc, w.tcw_out + 12 * (size_t)q, o);    // Tchildc * pKF->mTcwGBA
  }
  mc_centre(o, w.ow_out + 3 * (size_t)k);
}

// :734-765 for point p
PO_HD inline void mc_gba_point(const McGba& w, int p) {
  const float* x = w.xw + 3 * (size_t)p;
  float* o = w.xw_out + 3 * (size_t)p;
  o[0] = x[0], o[1] = x[1], o[2] = x[2];
  w.pt_changed[p] = 0;
  if (w.bad[p]) return;
  if (w.pt_optimised[p]) {
    const float* g = w.xw_gba + 3 * (size_t)p;
    o[0] = g[0], o[1] = g[1], o[2] = g[2];
    w.pt_changed[p] = 1;
    return;
  }
  const int k = w.ref_kf[p];
  if (k < 0) return;  // pRefKF->mnBAGlobalForKF != nLoopKF
  const float* B = w.tcw + 12 * (size_t)k;  // mTcwBefGBA
  // OPENCV: Rcw * X + tcw is one gemm with C: the double sum plus C in double, one rounding
  const float xc0 = (float)(mc_dot3(B[0], B[1], B[2], x[0], x[1], x[2]) + (double)B[3]);
  const float xc1 = (float)(mc_dot3(B[4], B[5], B[6], x[0], x[1], x[2]) + (double)B[7]);
  const float xc2 = (float)(mc_dot3(B[8], B[9], B[10], x[0], x[1], x[2]) + (double)B[11]);
  const float* T = w.tcw_out + 12 * (size_t)k;  // Rwc, twc of the new pose's stored inverse
  const float* O = w.ow_out + 3 * (size_t)k;
  o[0] = (float)(mc_dot3(T[0], T[4], T[8], xc0, xc1, xc2) + (double)O[0]);
  o[1] = (float)(mc_dot3(T[1], T[5], T[9], xc0, xc1, xc2) + (double)O[1]);
  o[2] = (float)(mc_dot3(T[2], T[6], T[10], xc0, xc1, xc2) + (double)O[2]);
  w.pt_changed[p] = 1;
}

// ---- the host side ------------------------------------------------------------------------------------
#define MC_PLAN_OK 0
#define MC_PLAN_PARENT 1  // a parent index outside -1 .. n_kf-1
#define MC_PLAN_CYCLE 2   // a cycle or a self-parent
#define MC_PLAN_ORIGIN 3  // an origin that is not optimised

// The order of the propagation: level d holds the keyframes d steps below their nearest optimised ancestor
// (level 0: the optimised ones), order[level_begin[d] .. level_begin[d+1]-1], ascending in index inside a
// level. A level depends on the one before it only.
struct McGbaPlan {
  std::vector<int> order, level_begin;
};

inline int mc_gba_plan(int n_kf, const int* parent, const uint8_t* optimised, McGbaPlan* P) {
  for (int k = 0; k < n_kf; k++) {
    if (parent[k] < -1 || parent[k] >= n_kf) return MC_PLAN_PARENT;
    if (parent[k] == -1 && !optimised[k]) return MC_PLAN_ORIGIN;
  }
  std::vector<int> state(n_kf, 0), depth(n_kf, -1), stack;  // state: 0 new, 1 on the walk, 2 done
  for (int k = 0; k < n_kf; k++) {
    int v = k;
    while (v >= 0 && state[v] == 0) {
      state[v] = 1;
      stack.push_back(v);
      v = parent[v];
    }
    if (v >= 0 && state[v] == 1) return MC_PLAN_CYCLE;
    while (!stack.empty()) {  // the parent of the top is done, or the top is an origin
      const int u = stack.back();
      stack.pop_back();
      depth[u] = optimised[u] ? 0 : depth[parent[u]] + 1;
      state[u] = 2;
    }
  }
  int levels = 0;
  for (int k = 0; k < n_kf; k++) levels = depth[k] + 1 > levels ? depth[k] + 1 : levels;
  P->level_begin.assign((size_t)levels + 1, 0);
  for (int k = 0; k < n_kf; k++) P->level_begin[(size_t)depth[k] + 1]++;
  for (int d = 0; d < levels; d++) P->level_begin[(size_t)d + 1] += P->level_begin[d];
  std::vector<int> at(P->level_begin.begin(), P->level_begin.end() - 1);
  P->order.assign(n_kf, 0);
  for (int k = 0; k < n_kf; k++) P->order[at[depth[k]]++] = k;
  return MC_PLAN_OK;
}

// The three walks, serially: what the kernels compute, in the reference's own order of work
inline void mc_host_normals(const McNd& w, int n_points, const float* xw, const uint8_t* bad) {
  for (int p = 0; p < n_points; p++) mc_nd_point(w, xw, bad, p);
}

inline void mc_host_loop(const McLoop& w) {
  for (int k = 0; k < w.n_kf; k++) mc_centre(w.tcw + 12 * (size_t)k, w.ow_old + 3 * (size_t)k);
  for (int i = 0; i < w.n_connected; i++) mc_loop_kf(w, i);
  for (int p = 0; p < w.n_points; p++) w.corrected_by[p] = MC_NONE;
  for (int t = 0; t < w.n_slots; t++) mc_loop_mark(w, t);
  for (int p = 0; p < w.n_points; p++) mc_loop_point(w, p);
}

inline void mc_host_gba(const McGba& w) {
  for (int i = 0; i < w.n_kf; i++) mc_gba_kf(w, w.order[i]);
  for (int p = 0; p < w.n_points; p++) mc_gba_point(w, p);
}
