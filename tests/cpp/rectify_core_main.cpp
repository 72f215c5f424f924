// Stand-alone host program over orb_slam2_2021_amd/csrc/orbfe_rectify_core.h and the _host entry points of
// include/orbfe_rectify.h (orbfe_rectify_host.cpp, compiled beside this file with ORBFE_RECTIFY_STANDALONE): no
// library, no GPU. tests/test_rectify_core.py builds it with ASan + UBSan, feeds it a binary case file and
// compares the binary answer, bit for bit, with tests/rectify_ref.py.
//
// usage: rectify_core_main CASES ANSWERS. Both files are sequences of little-endian records. A case starts with
// an int32 opcode; every answer starts with the int32 status of the call.
//   1 MAPS     int32 n_dist, has_R, rows, cols; double K[9], D[5], R[9], P3[9]
//              -> map1, map2 (rows * cols floats each) when the status is ORBFE_OK
//   2 ENTRIES  int32 rows, cols, src_rows, src_cols; float map1[rows * cols], map2[rows * cols]
//              -> rows * cols entries of 8 bytes
//   3 REMAP    int32 src_rows, src_cols, src_pitch, channels, dst_rows, dst_cols, map_pitch (bytes), row0, row1,
//              rgb, gray_mode, gray_out, dst_pitch; the source (src_rows * src_cols * channels bytes, packed);
//              map1, map2 (dst_rows * dst_cols floats each, packed)
//              -> the whole destination buffer, (row1 - row0 - 1) * dst_pitch + dst_cols * out_channels bytes,
//                 which was filled with 0xA5 before the call
//   4 BAD      -> int32 count, then the statuses of that many calls with one bad argument each
// Every buffer handed to the entry points has exactly the bytes its rows occupy, so that a read or write past the
// last row's last byte is an ASan error.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../orb_slam2_2021_amd/csrc/orbfe_rectify_core.h"

static FILE* in;
static FILE* out;

template <typename T>
static bool get(T* v, size_t n = 1) {
  return std::fread(v, sizeof(T), n, in) == n;
}
template <typename T>
static void put(const T* v, size_t n = 1) {
  std::fwrite(v, sizeof(T), n, out);
}

static int bad_calls(std::vector<int32_t>* st) {
  const double K[9] = {100, 0, 4, 0, 100, 3, 0, 0, 1}, D[5] = {0, 0, 0, 0, 0}, Z[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  std::vector<float> m1(48), m2(48);
  std::vector<uint8_t> src(48 * 3, 7), dst(48 * 3);
  std::vector<orbfe_rectify_entry> e(48);
  if (orbfe_rectify_maps_host(K, D, 4, nullptr, K, 6, 8, m1.data(), m2.data()) != ORBFE_OK) return 1;
  st->push_back(orbfe_rectify_maps_host(nullptr, D, 4, nullptr, K, 6, 8, m1.data(), m2.data()));
  st->push_back(orbfe_rectify_maps_host(K, D, 3, nullptr, K, 6, 8, m1.data(), m2.data()));
  st->push_back(orbfe_rectify_maps_host(K, D, 6, nullptr, K, 6, 8, m1.data(), m2.data()));
  st->push_back(orbfe_rectify_maps_host(K, D, 5, nullptr, Z, 6, 8, m1.data(), m2.data()));  // singular P * R
  st->push_back(orbfe_rectify_maps_host(K, D, 5, Z, K, 6, 8, m1.data(), m2.data()));
  st->push_back(orbfe_rectify_maps_host(K, D, 5, nullptr, K, 0, 8, m1.data(), m2.data()));
  st->push_back(orbfe_rectify_maps_host(K, D, 5, nullptr, K, 6, 8, nullptr, m2.data()));
  st->push_back(orbfe_rectify_entries_host(m1.data(), m2.data(), 6, 8, 6, 32767, e.data()));
  st->push_back(orbfe_rectify_entries_host(m1.data(), m2.data(), 6, 8, 0, 8, e.data()));
  st->push_back(orbfe_rectify_entries_host(m1.data(), nullptr, 6, 8, 6, 8, e.data()));
  auto remap = [&](int src_rows, int src_cols, size_t sp, int ch, size_t mp, int r0, int r1, int mode, size_t dp) {
    return orbfe_remap_host(src.data(), src_rows, src_cols, sp, ch, m1.data(), m2.data(), mp, 6, 8, r0, r1, 1, mode, 0,
                            dst.data(), dp);
  };
  if (remap(6, 8, 24, 3, 32, 0, 6, ORBFE_GRAY_SHIFT15, 24) != ORBFE_OK) return 1;
  st->push_back(remap(6, 8, 24, 2, 32, 0, 6, ORBFE_GRAY_SHIFT15, 24));    // channels
  st->push_back(remap(6, 8, 23, 3, 32, 0, 6, ORBFE_GRAY_SHIFT15, 24));    // source pitch below a row
  st->push_back(remap(6, 8, 24, 3, 28, 0, 6, ORBFE_GRAY_SHIFT15, 24));    // map pitch below a row
  st->push_back(remap(6, 8, 24, 3, 34, 0, 6, ORBFE_GRAY_SHIFT15, 24));    // map pitch not a multiple of 4
  st->push_back(remap(6, 8, 24, 3, 32, -1, 6, ORBFE_GRAY_SHIFT15, 24));   // row range
  st->push_back(remap(6, 8, 24, 3, 32, 0, 7, ORBFE_GRAY_SHIFT15, 24));
  st->push_back(remap(6, 8, 24, 3, 32, 4, 3, ORBFE_GRAY_SHIFT15, 24));
  st->push_back(remap(6, 8, 24, 3, 32, 0, 6, 2, 24));                     // gray mode
  st->push_back(remap(6, 8, 24, 3, 32, 0, 6, ORBFE_GRAY_SHIFT15, 23));    // destination pitch below a row
  st->push_back(remap(6, 32767, 24, 1, 32, 0, 6, ORBFE_GRAY_SHIFT15, 24));  // source beyond the short taps
  st->push_back(remap(0, 8, 24, 3, 32, 0, 6, ORBFE_GRAY_SHIFT15, 24));
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s CASES ANSWERS\n", argv[0]);
    return 2;
  }
  in = std::fopen(argv[1], "rb");
  out = std::fopen(argv[2], "wb");
  if (!in || !out) return 2;
  int32_t op;
  while (get(&op)) {
    if (op == 1) {
      int32_t h[4];
      double K[9], D[5], R[9], P3[9];
      if (!get(h, 4) || !get(K, 9) || !get(D, 5) || !get(R, 9) || !get(P3, 9)) return 2;
      const size_t n = (size_t)h[2] * h[3];
      std::vector<float> m1(n), m2(n);
      std::vector<double> d(D, D + (h[0] == 4 ? 4 : 5));  // exactly n_dist values where n_dist is valid
      const int32_t st = orbfe_rectify_maps_host(K, d.data(), h[0], h[1] ? R : nullptr, P3, h[2], h[3], m1.data(), m2.data());
      put(&st);
      if (st == ORBFE_OK) {
        put(m1.data(), n);
        put(m2.data(), n);
      }
    } else if (op == 2) {
      int32_t h[4];
      if (!get(h, 4)) return 2;
      const size_t n = (size_t)h[0] * h[1];
      std::vector<float> m1(n), m2(n);
      if (!get(m1.data(), n) || !get(m2.data(), n)) return 2;
      std::vector<orbfe_rectify_entry> e(n);
      const int32_t st = orbfe_rectify_entries_host(m1.data(), m2.data(), h[0], h[1], h[2], h[3], e.data());
      put(&st);
      if (st == ORBFE_OK) put(e.data(), n);
    } else if (op == 3) {
      int32_t h[13];
      if (!get(h, 13)) return 2;
      const int src_rows = h[0], src_cols = h[1], ch = h[3], dst_rows = h[4], dst_cols = h[5], row0 = h[7], row1 = h[8];
      const size_t sp = (size_t)h[2], mp = (size_t)h[6], dp = (size_t)h[12];
      const size_t srow = (size_t)src_cols * ch, mrow = (size_t)dst_cols * sizeof(float);
      const size_t drow = (size_t)dst_cols * rectify_out_channels(ch, h[11]);
      std::vector<uint8_t> src((size_t)(src_rows - 1) * sp + srow, 0xcd);
      for (int y = 0; y < src_rows; y++)
        if (!get(&src[(size_t)y * sp], srow)) return 2;
      // the maps live in float storage (aligned), rows mp bytes apart
      std::vector<float> m1(((size_t)(dst_rows - 1) * mp + mrow) / sizeof(float)), m2(m1.size());
      for (std::vector<float>* m : {&m1, &m2})
        for (int y = 0; y < dst_rows; y++)
          if (!get(reinterpret_cast<uint8_t*>(m->data()) + (size_t)y * mp, mrow)) return 2;
      std::vector<uint8_t> dst(row1 > row0 ? (size_t)(row1 - row0 - 1) * dp + drow : 0, 0xA5);
      const int32_t st = orbfe_remap_host(src.data(), src_rows, src_cols, sp, ch, m1.data(), m2.data(), mp, dst_rows,
                                          dst_cols, row0, row1, h[9], h[10], h[11], dst.data(), dp);
      put(&st);
      if (st == ORBFE_OK) put(dst.data(), dst.size());
    } else if (op == 4) {
      std::vector<int32_t> st;
      if (bad_calls(&st) != 0) return 4;
      const int32_t n = (int32_t)st.size();
      put(&n);
      put(st.data(), st.size());
    } else {
      return 2;
    }
  }
  std::fclose(out);
  return 0;
}
