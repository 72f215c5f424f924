// orbfe_cull_core.h -- the per-item rules of the two cullings (include/orbfe_covis.h):
// LocalMapping::KeyFrameCulling (LocalMapping.cc:640-706) with the EraseObservation cascade of
// KeyFrame::SetBadFlag (KeyFrame.cc:486-488, MapPoint.cc:141-198) and LocalMapping::MapPointCulling
// (LocalMapping.cc:174-209), as host/device inline functions over one item each (a row slot, an
// observer, a candidate, a recent point), and the serial composition of them on the host
// (cull_host_keyframes). Used by the kernels of orbfe_covis.hip and by the stand-alone host program
// tests/cpp/cull_core_test.cpp. Not part of the C ABI. tests/culling_ref.py reaches the same
// results a second way, with the reference's containers.
//
// All arithmetic is integer but two places: 0.9 * nMPs is one double multiply followed by one double
// compare (never contracted: there is nothing to contract with), and the found ratio is one
// correctly rounded float divide of two ints converted to float.
#pragma once
#include <stdint.h>

#include <vector>

#if defined(__HIPCC__)
#define CULL_HD __host__ __device__
#else
#define CULL_HD
#endif

#define CULL_ATTR_OCTAVE 0x1f
#define CULL_ATTR_STEREO 0x20
#define CULL_ATTR_FAR 0x40

enum { CULL_KEPT = 0, CULL_CULLED = 1, CULL_NOT_ERASE = 2, CULL_SKIPPED = 3 };
enum { CULL_PT_STAYS = 0, CULL_PT_WAS_BAD = 1, CULL_PT_RATIO = 2, CULL_PT_OBS = 3, CULL_PT_AGE = 4 };

// LocalMapping.cc:663-673: does slot i of the candidate's row reach nMPs++? p: the slot's point id
// (< 0: none), bad: the point's isBad(), attr: the candidate's attribute byte at the slot.
CULL_HD inline bool cull_slot_counted(int p, int bad, uint8_t attr, int monocular) {
  if (p < 0) return false;
  if (bad) return false;
  if (!monocular && (attr & CULL_ATTR_FAR)) return false;
  return true;
}

// MapPoint.cc:135-138: what one observer adds to nObs; attr is the observer's byte at its recorded slot.
CULL_HD inline int cull_weight(uint8_t attr) { return (attr & CULL_ATTR_STEREO) ? 2 : 1; }

// LocalMapping.cc:685-687: scaleLeveli <= scaleLevel + 1
CULL_HD inline bool cull_gate(uint8_t attr_observer, uint8_t attr_candidate_slot) {
  return (int)(attr_observer & CULL_ATTR_OCTAVE) <= (int)(attr_candidate_slot & CULL_ATTR_OCTAVE) + 1;
}

// :674 and :694. observations: Observations(), the candidate included; gated_others: the observers other
// than the candidate that pass cull_gate (the break at :690 only stops the count early).
CULL_HD inline bool cull_slot_redundant(int observations, int gated_others) {
  return observations > 3 && gated_others >= 3;
}

// :703: an int against a double product
CULL_HD inline bool cull_keyframe_redundant(int n_redundant, int n_mps) {
  const double line = 0.9 * (double)n_mps;
  return (double)n_redundant > line;
}

// :652, :703-704 and KeyFrame.cc:473-479
CULL_HD inline int cull_decision(int n_redundant, int n_mps, int not_erase) {
  if (!cull_keyframe_redundant(n_redundant, n_mps)) return CULL_KEPT;
  return not_erase ? CULL_NOT_ERASE : CULL_CULLED;
}

// MapPoint.cc:160: nObs after EraseObservation
CULL_HD inline bool cull_point_goes_bad(int observations_left) { return observations_left <= 2; }

// LocalMapping.cc:190-207 for one recent point. cur, first: keyframe ids below 2^31 (the caller checks),
// so the reference's (int) casts are exact.
CULL_HD inline int cull_point_action(int bad, int32_t found, int32_t visible, int64_t cur, int64_t first,
                                     int observations, int monocular) {
  if (bad) return CULL_PT_WAS_BAD;
  const float ratio = (float)found / (float)visible;  // 0/0: NaN, never < ; x/0: +-inf
  if (ratio < 0.25f) return CULL_PT_RATIO;
  const int age = (int)cur - (int)first;
  const int th = monocular ? 2 : 3;
  if (age >= 2 && observations <= th) return CULL_PT_OBS;
  if (age >= 3) return CULL_PT_AGE;
  return CULL_PT_STAYS;
}

// ---- the serial composition on the host ------------------------------------------------------
// The table as the device holds it: rows by ascending mnId (row r: ids[r]), one attribute byte per slot,
// one bad flag per point id. Observers are derived by the rules of include/orbfe_covis.h.
struct CullHostTable {
  std::vector<int64_t> ids;                  // ascending
  std::vector<std::vector<int32_t>> rows;    // point id per slot, -1: none
  std::vector<std::vector<uint8_t>> attrs;
  std::vector<uint8_t> live;                 // 0: culled
  std::vector<uint8_t> bad;                  // [n_points]
};

struct CullHostResult {
  std::vector<uint8_t> decision;
  std::vector<int32_t> n_mps, n_redundant;
  std::vector<int32_t> bad_begin, bad_points;
};

// (row, lowest slot) of every live observer of p, ascending in mnId
inline void cull_host_observers(const CullHostTable& t, int p, std::vector<int>* rows, std::vector<int>* slots) {
  rows->clear();
  slots->clear();
  for (size_t r = 0; r < t.rows.size(); r++) {
    if (!t.live[r]) continue;
    for (size_t s = 0; s < t.rows[r].size(); s++)
      if (t.rows[r][s] == p) {
        rows->push_back((int)r);
        slots->push_back((int)s);
        break;
      }
  }
}

// cand: row index per candidate, in the caller's order. Mutates t as the reference mutates the map.
inline void cull_host_keyframes(CullHostTable* t, const std::vector<int>& cand, const std::vector<uint8_t>& not_erase,
                                int monocular, CullHostResult* out) {
  const size_t n = cand.size();
  out->decision.assign(n, 0);
  out->n_mps.assign(n, 0);
  out->n_redundant.assign(n, 0);
  out->bad_begin.assign(n + 1, 0);
  out->bad_points.clear();
  std::vector<int> orow, oslot;
  for (size_t c = 0; c < n; c++) {
    const int r = cand[c];
    out->bad_begin[c] = (int32_t)out->bad_points.size();
    if (t->ids[r] == 0) {
      out->decision[c] = CULL_SKIPPED;
      continue;
    }
    int n_mps = 0, n_red = 0;
    for (size_t i = 0; i < t->rows[r].size(); i++) {
      const int p = t->rows[r][i];
      const uint8_t a = t->attrs[r][i];
      if (!cull_slot_counted(p, p >= 0 ? t->bad[p] : 0, a, monocular)) continue;
      n_mps++;
      cull_host_observers(*t, p, &orow, &oslot);
      int obs = 0, gated = 0;
      for (size_t k = 0; k < orow.size(); k++) {
        const uint8_t ao = t->attrs[orow[k]][oslot[k]];
        obs += cull_weight(ao);
        if (orow[k] != r && cull_gate(ao, a)) gated++;
      }
      if (cull_slot_redundant(obs, gated)) n_red++;
    }
    out->n_mps[c] = n_mps;
    out->n_redundant[c] = n_red;
    const int d = cull_decision(n_red, n_mps, not_erase[c]);
    out->decision[c] = (uint8_t)d;
    if (d != CULL_CULLED) continue;
    t->live[r] = 0;  // EraseObservation(this) on every point, in slot order
    for (size_t i = 0; i < t->rows[r].size(); i++) {
      const int p = t->rows[r][i];
      if (p < 0 || t->bad[p]) continue;
      bool first = true;
      for (size_t j = 0; j < i; j++) first = first && t->rows[r][j] != p;
      if (!first) continue;
      cull_host_observers(*t, p, &orow, &oslot);
      int obs = 0;
      for (size_t k = 0; k < orow.size(); k++) obs += cull_weight(t->attrs[orow[k]][oslot[k]]);
      if (!cull_point_goes_bad(obs)) continue;
      t->bad[p] = 1;
      out->bad_points.push_back(p);
      for (size_t k = 0; k < orow.size(); k++) t->rows[orow[k]][oslot[k]] = -1;  // EraseMapPointMatch(mit->second)
    }
  }
  out->bad_begin[n] = (int32_t)out->bad_points.size();
}
