// pnp_core_main.cpp -- orbfe_pnp_core.h on the host: EPnP (compute_pose) over the samples of a text
// file, result bits printed for tests/test_pnp_ref.py to compare with tests/pnp_ref.py. Built with
// -fsanitize=address,undefined; no GPU, no library.
//
// Input: the sample count, then per sample "n fx fy cx cy" and n lines "X Y Z u v"; every real is
// the hex bit pattern of a float. Output per sample: "N flags" and the 12 doubles of R, t as hex.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../orb_slam2_2021_amd/csrc/orbfe_pnp_core.h"

static bool read_float(FILE* f, float* out) {
  unsigned bits = 0;
  if (fscanf(f, "%x", &bits) != 1) return false;
  memcpy(out, &bits, 4);
  return true;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  int count = 0;
  if (fscanf(f, "%d", &count) != 1) return 2;
  for (int s = 0; s < count; s++) {
    int n = 0;
    if (fscanf(f, "%d", &n) != 1 || n < 4 || n > 4096) return 2;
    float kf[4];
    for (int i = 0; i < 4; i++)
      if (!read_float(f, &kf[i])) return 2;
    const double K[4] = {kf[0], kf[1], kf[2], kf[3]};
    std::vector<double> pws(3 * n), us(2 * n), alphas(4 * n), pcs(3 * n);
    for (int i = 0; i < n; i++) {
      float v[5];
      for (int j = 0; j < 5; j++)
        if (!read_float(f, &v[j])) return 2;
      for (int j = 0; j < 3; j++) pws[3 * i + j] = v[j];
      us[2 * i] = v[3];
      us[2 * i + 1] = v[4];
    }
    PnpWork w;
    memset(&w, 0, sizeof(w));
    double R[9], t[3];
    int N = 0;
    unsigned flags = 0;
    pnp_compute_pose(PnpHostGroup(), w, n, pws.data(), us.data(), alphas.data(), pcs.data(), K, R, t, &N, &flags);
    printf("%d %u", N, flags);
    for (int i = 0; i < 12; i++) {
      const double d = i < 9 ? R[i] : t[i - 9];
      unsigned long long bits;
      memcpy(&bits, &d, 8);
      printf(" %016llx", bits);
    }
    printf("\n");
  }
  fclose(f);
  return 0;
}
