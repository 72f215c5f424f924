// orbfe_covis_view.h -- a read-only view of an orbfe_covis handle's device arrays for the other
// handles of the library that walk its rows (orbfe_gridmap.hip). Not part of the C ABI.
#pragma once
#include <stdint.h>

#include <vector>

struct orbfe_covis;

struct CovisRowsView {
  int device;              // < 0: a host-only handle, every pointer NULL
  const int32_t* rows;     // [M * S] point id per slot, -1: none
  const int32_t* row_n;    // [M]
  const uint8_t* bad;      // [P]
  const uint8_t* geo_rec;  // [P * 64] descriptor 32 | pos 12 | normal 12 | min 4 | max 4; NULL: never allocated
  const uint8_t* geo_state;  // [P] orbfe_localmap_core::kPresent when the record was set; NULL with geo_rec
  int M, S, P;
};

// The rows of n_kf stored keyframes (repeats allowed) and their stored lengths, after the checks of
// orbfe_covis_distinct_points: n_kf outside 1..4096 ORBFE_ERR_ARG / ORBFE_ERR_CAPACITY, an id that is not
// stored ORBFE_ERR_ARG.
int orbfe_covis_rows_view(orbfe_covis* h, int n_kf, const int64_t* kf_ids, std::vector<int32_t>* list_rows,
                          std::vector<int32_t>* row_len, CovisRowsView* view);
