// The buffer plans of the five batched solvers (sim3, pnp, initializer, poseopt, optsim3) and the small
// helpers of orb_slam2_2021_amd/csrc/orbfe_stage.h, on the host alone: built with ASan + UBSan by
// tests/test_stage_layout.py, no GPU and no library.
//
// Every plan is laid out twice, as a handle does it: once over counting blocks, then over heap buffers
// of exactly the counted size. Checked per plan: (a) every offset is a multiple of 256 and the regions are
// disjoint and ascending, (b) every byte of every region can be written (ASan sees an overrun), (d) the
// plan fits the sizes a handle with these bounds allocates, (e) every offset is where the take order this
// file restates puts it. Checked per handle: (c) the allocated sizes equal the closed formulas restated
// here by hand.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../orb_slam2_2021_amd/csrc/orbfe_init_core.h"
#include "../../orb_slam2_2021_amd/csrc/orbfe_optsim3_core.h"
#include "../../orb_slam2_2021_amd/csrc/orbfe_pnp_core.h"
#include "../../orb_slam2_2021_amd/csrc/orbfe_poseopt_core.h"
#include "../../orb_slam2_2021_amd/csrc/orbfe_sim3_core.h"
#include "../../orb_slam2_2021_amd/csrc/orbfe_stage.h"

static long g_checks = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    g_checks++;                                                       \
    if (!(cond)) {                                                    \
      printf("%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
      exit(1);                                                        \
    }                                                                 \
  } while (0)

// the kernels read the records as they are
static_assert(sizeof(Sim3Dev) == 184 && sizeof(PnpDev) == 240 && sizeof(InitDev) == 208 && sizeof(PoDev) == 152 &&
                  sizeof(OsDev) == 264,
              "record sizes");

// the alignment rule, restated
static size_t al(size_t b) { return (b + 255) / 256 * 256; }

// One buffer of a plan: the heap block of exactly the counted size and the offset the next region must
// have by the restated take order
struct Walk {
  uint8_t* buf;
  size_t total, expect;
  bool aligned;
  Walk(size_t total_, size_t first, bool aligned_ = true)
      : buf((uint8_t*)malloc(total_ ? total_ : 1)), total(total_), expect(first), aligned(aligned_) {}
  ~Walk() { free(buf); }
  void region(unsigned long long off, size_t bytes) {
    CHECK(off == expect);                   // (e), and with it ascending and disjoint (a)
    if (aligned) CHECK(off % 256 == 0);     // (a)
    CHECK(off + bytes <= total);            // (b), before ASan would say so
    memset(buf + off, 0xA5, bytes);         // (b)
    expect += aligned ? al(bytes) : bytes;
  }
  OrbfeStage stage() const {
    OrbfeStage s;
    s.d = s.h = buf;
    s.cap = total;
    return s;
  }
};

struct Prob {
  size_t n, e;
};

// ---------------------------------------------------------------------------------------------- sim3
static void sim3_plan(const std::vector<Prob>& probs, bool has_hyp, size_t in_bound, size_t res_bound) {
  const size_t S = probs.size();
  OrbfeStage cin, cres;
  Sim3Dev d;
  cin.take(sizeof(Sim3Dev) * S);
  for (const Prob& p : probs) sim3_layout(cin, cres, p.n, p.e, has_hyp, d);
  CHECK(cin.off <= in_bound && cres.off <= res_bound);  // (d)
  Walk win(cin.off, al(sizeof(Sim3Dev) * S)), wres(cres.off, 0);
  OrbfeStage in = win.stage(), res = wres.stage();
  Sim3Dev* table;
  CHECK((uint8_t*)in.take<Sim3Dev>(S, &table) == win.buf && (uint8_t*)table == win.buf);
  for (size_t s = 0; s < S; s++) {
    const size_t n = probs[s].n, e = probs[s].e, w = (n + 63) / 64;
    memset(&d, 0, sizeof(d));
    sim3_layout(in, res, n, e, has_hyp, d);
    table[s] = d;
    win.region(d.in_x1, 12 * n);
    win.region(d.in_x2, 12 * n);
    win.region(d.in_max1, 4 * n);
    win.region(d.in_max2, 4 * n);
    if (has_hyp) {
      win.region(d.in_t12, 48 * e);
      win.region(d.in_t21, 48 * e);
      CHECK(d.in_rand == 0);
    } else {
      win.region(d.in_rand, 12 * e);
      CHECK(d.in_t12 == 0 && d.in_t21 == 0);
    }
    wres.region(d.o_mask, 8 * w * e);
    wres.region(d.o_t12, 48 * e);
    wres.region(d.o_t21, 48 * e);
    wres.region(d.o_r, 36 * e);
    wres.region(d.o_t, 12 * e);
    wres.region(d.o_s, 4 * e);
    wres.region(d.o_cnt, 4 * e);
    wres.region(d.o_sel, 32);
  }
  CHECK(win.expect == in.off && in.off == cin.off && wres.expect == res.off && res.off == cres.off);
}

// ----------------------------------------------------------------------------------------------- pnp
static void pnp_plan(const std::vector<Prob>& probs, size_t in_bound, size_t res_bound, size_t ws_bound) {
  const size_t S = probs.size(), r = 16;
  OrbfeStage cin, cres, cws;
  PnpDev d;
  cin.take(sizeof(PnpDev) * S);
  for (const Prob& p : probs) pnp_layout(cin, cres, cws, p.n, p.e, d);
  CHECK(cin.off <= in_bound && cres.off <= res_bound && cws.off <= ws_bound);  // (d)
  Walk win(cin.off, al(sizeof(PnpDev) * S)), wres(cres.off, 0), wws(cws.off, 0, false);
  OrbfeStage in = win.stage(), res = wres.stage(), ws = wws.stage();
  PnpDev* table;
  in.take<PnpDev>(S, &table);
  for (size_t s = 0; s < S; s++) {
    const size_t n = probs[s].n, e = probs[s].e, w = (n + 63) / 64;
    memset(&d, 0, sizeof(d));
    pnp_layout(in, res, ws, n, e, d);
    table[s] = d;
    win.region(d.in_p3d, 12 * n);
    win.region(d.in_p2d, 8 * n);
    win.region(d.in_max, 4 * n);
    win.region(d.in_rand, 16 * e);
    wres.region(d.o_mask, 8 * w * e);
    wres.region(d.o_r, 72 * e);
    wres.region(d.o_t, 24 * e);
    wres.region(d.o_tcw, 48 * e);
    wres.region(d.o_N, 4 * e);
    wres.region(d.o_flags, 4 * e);
    wres.region(d.o_cnt, 4 * e);
    wres.region(d.o_slot, 4 * e);
    wres.region(d.o_rec, 4 * r);
    wres.region(d.o_rmask, 8 * w * r);
    wres.region(d.o_rr, 72 * r);
    wres.region(d.o_rt, 24 * r);
    wres.region(d.o_rtcw, 48 * r);
    wres.region(d.o_rN, 4 * r);
    wres.region(d.o_rflags, 4 * r);
    wres.region(d.o_rcnt, 4 * r);
    wres.region(d.o_sel, 32);
    CHECK(d.ws % 8 == 0);  // the kernel indexes doubles from ws / 8
    wws.region(d.ws, r * 12 * 8 * n);
  }
  CHECK(win.expect == in.off && in.off == cin.off && wres.expect == res.off && res.off == cres.off &&
        wws.expect == ws.off && ws.off == cws.off);
}

// ---------------------------------------------------------------------------------------------- init
struct InitProb {
  size_t n1, n2, m, e;
};

static void init_plan(const std::vector<InitProb>& probs, size_t in_bound, size_t res_bound, size_t ws_bound) {
  const size_t S = probs.size();
  OrbfeStage cin, cres, cws;
  InitDev d;
  cin.take(sizeof(InitDev) * S);
  for (const InitProb& p : probs) init_layout(cin, cres, cws, p.n1, p.n2, p.m, p.e, d);
  CHECK(cin.off <= in_bound && cres.off <= res_bound && cws.off <= ws_bound);  // (d)
  Walk win(cin.off, al(sizeof(InitDev) * S)), wres(cres.off, 0), wws(cws.off, 0);
  OrbfeStage in = win.stage(), res = wres.stage(), ws = wws.stage();
  InitDev* table;
  in.take<InitDev>(S, &table);
  for (size_t s = 0; s < S; s++) {
    const size_t n1 = probs[s].n1, n2 = probs[s].n2, m = probs[s].m, e = probs[s].e, w = (m + 63) / 64;
    memset(&d, 0, sizeof(d));
    init_layout(in, res, ws, n1, n2, m, e, d);
    table[s] = d;
    win.region(d.in_k1, 8 * n1);
    win.region(d.in_k2, 8 * n2);
    win.region(d.in_m1, 4 * m);
    win.region(d.in_m2, 4 * m);
    win.region(d.in_rand, 32 * e);
    wres.region(d.o_nrm, 2 * 16);
    wres.region(d.o_sh, 4 * e);
    wres.region(d.o_sf, 4 * e);
    wres.region(d.o_sel, sizeof(InitSel));
    wres.region(d.o_mh, 8 * w);
    wres.region(d.o_mf, 8 * w);
    wres.region(d.o_p3d, 12 * n1);
    wres.region(d.o_tri, n1);
    wws.region(d.w_models, 108 * e);
    wws.region(d.w_masks, 16 * w * e);
    wws.region(d.w_p3d, 96 * n1);
    wws.region(d.w_good, 8 * n1);
    wws.region(d.w_cos, 32 * m);
  }
  CHECK(win.expect == in.off && in.off == cin.off && wres.expect == res.off && res.off == cres.off &&
        wws.expect == ws.off && ws.off == cws.off);
}

// ------------------------------------------------------------------------------------ poseopt, optsim3
static void po_plan(const std::vector<Prob>& probs, size_t in_bound, size_t res_bound) {
  const size_t S = probs.size();
  OrbfeStage cin, cres;
  PoDev d;
  cin.take(sizeof(PoDev) * S);
  for (const Prob& p : probs) po_layout(cin, cres, p.n, d);
  CHECK(cin.off <= in_bound && cres.off <= res_bound);  // (d)
  Walk win(cin.off, al(sizeof(PoDev) * S)), wres(cres.off, 0);
  OrbfeStage in = win.stage(), res = wres.stage();
  PoDev* table;
  in.take<PoDev>(S, &table);
  for (size_t s = 0; s < S; s++) {
    const size_t n = probs[s].n;
    memset(&d, 0, sizeof(d));
    po_layout(in, res, n, d);
    table[s] = d;
    win.region(d.in_valid, n);
    win.region(d.in_xw, 12 * n);
    win.region(d.in_kp, 8 * n);
    win.region(d.in_ur, 4 * n);
    win.region(d.in_is2, 4 * n);
    wres.region(d.o_out, sizeof(PoOut));
    wres.region(d.o_mask, 8 * ((n + 63) / 64));
  }
  CHECK(win.expect == in.off && in.off == cin.off && wres.expect == res.off && res.off == cres.off);
}

static void os_plan(const std::vector<Prob>& probs, size_t in_bound, size_t res_bound) {
  const size_t S = probs.size();
  OrbfeStage cin, cres;
  OsDev d;
  cin.take(sizeof(OsDev) * S);
  for (const Prob& p : probs) os_layout(cin, cres, p.n, d);
  CHECK(cin.off <= in_bound && cres.off <= res_bound);  // (d)
  Walk win(cin.off, al(sizeof(OsDev) * S)), wres(cres.off, 0);
  OrbfeStage in = win.stage(), res = wres.stage();
  OsDev* table;
  in.take<OsDev>(S, &table);
  for (size_t s = 0; s < S; s++) {
    const size_t n = probs[s].n;
    memset(&d, 0, sizeof(d));
    os_layout(in, res, n, d);
    table[s] = d;
    win.region(d.in_valid, n);
    win.region(d.in_p1, 12 * n);
    win.region(d.in_p2, 12 * n);
    win.region(d.in_kp1, 8 * n);
    win.region(d.in_kp2, 8 * n);
    win.region(d.in_is1, 4 * n);
    win.region(d.in_is2, 4 * n);
    wres.region(d.o_out, sizeof(OsOut));
    wres.region(d.o_mask, 8 * ((n + 63) / 64));
  }
  CHECK(win.expect == in.off && in.off == cin.off && wres.expect == res.off && res.off == cres.off);
}

// The plans of S problems over the sizes that can go wrong: each (n, e) for all S problems, and one plan
// that mixes them; n runs over the minimal set, 63, 64 and 65 = the bound, e over 0, 1 and 3 = the bound
static std::vector<std::vector<Prob>> plans(size_t S, size_t min_set) {
  const size_t ns[4] = {min_set, 63, 64, 65}, es[3] = {0, 1, 3};
  std::vector<std::vector<Prob>> out;
  std::vector<Prob> mixed;
  for (size_t n : ns)
    for (size_t e : es) {
      out.push_back(std::vector<Prob>(S, Prob{n, e}));
      if (mixed.size() < S && n != 65 && e != 0) mixed.push_back(Prob{n, e});
    }
  while (mixed.size() < S) mixed.push_back(Prob{65, 3});
  out.push_back(mixed);
  return out;
}

static void layouts() {
  const size_t C = 65, H = 3, r = 16, w = (C + 63) / 64;
  for (size_t S : {(size_t)1, (size_t)3}) {
    size_t in_b, res_b, ws_b;
    // (c): the sizes of a handle with max_solvers = S, max_corr = C, max_hyp = H, by the closed formulas
    sim3_plan_bounds(S, C, H, &in_b, &res_b);
    CHECK(in_b == al(184 * S) + S * (2 * al(12 * C) + 2 * al(4 * C) + std::max(al(12 * H), 2 * al(48 * H))));
    CHECK(res_b == S * (al(8 * w * H) + 2 * al(48 * H) + al(36 * H) + al(12 * H) + 2 * al(4 * H) + 256));
    for (const auto& p : plans(S, 3))
      for (bool has_hyp : {false, true}) sim3_plan(p, has_hyp, in_b, res_b);

    pnp_plan_bounds(S, C, H, &in_b, &res_b, &ws_b);
    CHECK(in_b == al(240 * S) + S * (al(12 * C) + al(8 * C) + al(4 * C) + al(16 * H)));
    CHECK(res_b == S * (al(8 * w * H) + al(72 * H) + al(24 * H) + al(48 * H) + 4 * al(4 * H) + al(4 * r) + al(8 * w * r) +
                        al(72 * r) + al(24 * r) + al(48 * r) + 3 * al(4 * r) + al(4 * 8)));
    CHECK(ws_b == S * 16 * 12 * 8 * C);
    for (const auto& p : plans(S, 4)) pnp_plan(p, in_b, res_b, ws_b);

    // max_keys = 65, max_matches = 64 (w = 1), max_hyp = 3
    const size_t K = 65, M = 64, wm = 1;
    init_plan_bounds(S, K, M, H, &in_b, &res_b, &ws_b);
    CHECK(in_b == al(208 * S) + S * (2 * al(8 * K) + 2 * al(4 * M) + al(32 * H)));
    CHECK(res_b == S * (al(2 * 16) + 2 * al(4 * H) + al(sizeof(InitSel)) + 2 * al(8 * wm) + al(12 * K) + al(K)));
    CHECK(ws_b == S * (al(108 * H) + al(16 * wm * H) + al(96 * K) + al(8 * K) + al(32 * M)));
    CHECK(sizeof(InitNorm) == 16 && sizeof(InitSel) == 568);  // 8 + 8 + 8 + 4 + 9 + 9 + 72 + 24 words
    std::vector<InitProb> mixed;
    for (size_t m : {(size_t)8, (size_t)63, (size_t)64})
      for (size_t e : {(size_t)0, (size_t)1, (size_t)3}) {
        // n1 != n2 and N < n1 in both orders, and the bounds themselves
        const InitProb ps[3] = {{65, m, m, e}, {m + 1, 65, m, e}, {65, 65, m, e}};
        for (const InitProb& p : ps) init_plan(std::vector<InitProb>(S, p), in_b, res_b, ws_b);
        if (mixed.size() < S && e != 0) mixed.push_back(ps[mixed.size() % 2]);
      }
    init_plan(mixed, in_b, res_b, ws_b);
    // max_matches = max_keys = 65: two mask words
    init_plan_bounds(S, 65, 65, H, &in_b, &res_b, &ws_b);
    CHECK(res_b == S * (al(2 * 16) + 2 * al(4 * H) + al(560) + 2 * al(8 * 2) + al(12 * 65) + al(65)));
    CHECK(ws_b == S * (al(108 * H) + al(16 * 2 * H) + al(96 * 65) + al(8 * 65) + al(32 * 65)));
    init_plan(std::vector<InitProb>(S, InitProb{65, 65, 65, 3}), in_b, res_b, ws_b);

    po_plan_bounds(S, C, &in_b, &res_b);
    CHECK(in_b == al(152 * S) + S * (al(C) + al(12 * C) + al(8 * C) + 2 * al(4 * C)));
    CHECK(res_b == S * (al(sizeof(PoOut)) + al(8 * ((C + 63) / 64))));
    for (size_t n : {(size_t)0, (size_t)1, (size_t)63, (size_t)64, (size_t)65})
      po_plan(std::vector<Prob>(S, Prob{n, 0}), in_b, res_b);

    os_plan_bounds(S, C, &in_b, &res_b);
    CHECK(in_b == al(264 * S) + S * (al(C) + 2 * al(12 * C) + 2 * al(8 * C) + 2 * al(4 * C)));
    CHECK(res_b == S * (al(sizeof(OsOut)) + al(8 * ((C + 63) / 64))));
    for (size_t n : {(size_t)0, (size_t)1, (size_t)63, (size_t)64, (size_t)65})
      os_plan(std::vector<Prob>(S, Prob{n, 0}), in_b, res_b);
  }
}

// ------------------------------------------------------------------------------------------- helpers
static void al256_and_stage() {
  CHECK(orbfe_al256(0) == 0 && orbfe_al256(1) == 256 && orbfe_al256(255) == 256 && orbfe_al256(256) == 256 &&
        orbfe_al256(257) == 512);
  // a counting block hands out null addresses and counts what a real one uses
  OrbfeStage c;
  float some = 0;
  float *f = &some, *hf = &some;
  c.take(f, 3);
  CHECK(f == nullptr && c.off == 256);
  CHECK(c.take<float>(65, &hf) == nullptr && hf == nullptr && c.off == 768);
  // put copies through the host side and returns the device side at the same offset
  std::vector<uint8_t> host(512), dev(512);
  OrbfeStage s;
  s.h = host.data(), s.d = dev.data(), s.cap = 512;
  const int32_t src[3] = {7, 8, 9};
  CHECK((const uint8_t*)s.put(src, 3) == dev.data() && memcmp(host.data(), src, 12) == 0);
  CHECK((const uint8_t*)s.put(src, 0) == dev.data() + 256 && s.off == 256);  // an empty array takes no room
  CHECK((const uint8_t*)s.put(src + 1, 2) == dev.data() + 256 && memcmp(host.data() + 256, src + 1, 8) == 0 && s.off == 512);
}

static void draws() {
  for (int set : {3, 4, 8}) {
    const int n = set + 2, n_hyp = 2;
    for (int i = 0; i < set; i++) {
      std::vector<int32_t> d((size_t)set * n_hyp, 0);  // exactly n_hyp sets: ASan sees a read past them
      int32_t& at = d[(size_t)set * (n_hyp - 1) + i];
      CHECK(ransac_check_draws(d.data(), n_hyp, set, n));
      at = -1;
      CHECK(!ransac_check_draws(d.data(), n_hyp, set, n));
      at = n - 1 - i;
      CHECK(ransac_check_draws(d.data(), n_hyp, set, n));
      at = n - i;
      CHECK(!ransac_check_draws(d.data(), n_hyp, set, n));
      CHECK(ransac_check_draws(d.data(), n_hyp - 1, set, n));  // the bad draw is outside the first n_hyp - 1 sets
    }
    CHECK(ransac_check_draws(nullptr, 0, set, n));
  }
}

static void max_its() {
  // min_inliers == n: one iteration, whatever epsilon and probability say
  CHECK(ransac_max_its(40, 40, 1.0f, 0.99, 300) == 1);
  // epsilon = 0.5, p = 0.99: ln(0.01) / ln(0.875) = -4.60517 / -0.133531 = 34.49, so 35; capped by max_iterations
  CHECK(ransac_max_its(40, 20, 0.5f, 0.99, 300) == 35);
  CHECK(ransac_max_its(40, 20, 0.5f, 0.99, 20) == 20);
  // epsilon = 1e-4: ln(0.01) / ln(1 - 1e-12) is about 4.6e12, outside int; x86's conversion gives INT_MIN,
  // min(INT_MIN, 300) stays there and the floor of 1 holds (a saturating conversion would say 300)
  CHECK(ransac_max_its(40000, 4, 1e-4f, 0.99, 300) == 1);
  // epsilon so small that 1 - epsilon^3 == 1: ln(0.01) / 0 = -inf, the same rule
  CHECK(ransac_max_its(40000, 4, 1e-8f, 0.99, 300) == 1);
  // probability 0: ln(1) / ln(0.875) = -0, ceil keeps it, (int) gives 0, held to 1
  CHECK(ransac_max_its(40, 20, 0.5f, 0.0, 300) == 1);
  // probability 1: ln(0) / ln(0.875) = +inf, out of range, INT_MIN, held to 1
  CHECK(ransac_max_its(40, 20, 0.5f, 1.0, 300) == 1);
}

static void masks() {
  const int src_words = 2;
  const size_t count = 3;
  std::vector<uint8_t> src(8 * src_words * count);  // exactly count masks
  for (size_t i = 0; i < src.size(); i++) src[i] = (uint8_t)(i * 37 + 1);
  for (int dst_words : {2, 3, 5}) {
    std::vector<uint64_t> dst((size_t)dst_words * count, ~0ull);  // exactly count rows
    orbfe_unpack_masks(dst.data(), dst_words, src.data(), src_words, count);
    for (size_t k = 0; k < count; k++) {
      CHECK(memcmp(&dst[k * dst_words], &src[8 * src_words * k], 8 * src_words) == 0);
      for (int w = src_words; w < dst_words; w++) CHECK(dst[k * dst_words + w] == 0);
    }
  }
  uint64_t one = ~0ull;
  orbfe_unpack_masks(&one, 1, src.data(), 0, 1);  // n == 0: no source word, the row is cleared
  CHECK(one == 0);
  orbfe_unpack_masks(nullptr, 2, nullptr, 2, 0);  // nothing to unpack
}

int main() {
  al256_and_stage();
  layouts();
  draws();
  max_its();
  masks();
  printf("stage_layout_test: ok, %ld checks\n", g_checks);
  return 0;
}
