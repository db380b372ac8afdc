// resample_div_check.cpp — the limb arithmetic of the resampling points on the host.
//
// csrc/fw_resample_limbs.h holds fw_rsm_point as a plain function, so this program compiles the
// text the device compiles and compares it with unsigned __int128 (which the host has):
//   random     j < C <= 2^20, u < 2^32, T <= 2^50, all random (C also forced to powers of two
//              and to the bound)
//   extreme    every combination of the corner values of j, u, T and C
//   ascending  p_0 <= p_1 <= .. <= p_{C-1} < T along whole random populations
// One line per family: "<name> cases <n> mismatches <m>"; exit status 1 on any mismatch.
#include <cstdint>
#include <cstdio>

#include "../flipcomplexityempirical_amd/csrc/fw_resample_limbs.h"

namespace {

uint64_t state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {  // splitmix64
  uint64_t z = (state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

uint64_t exact(uint32_t j, uint32_t u, uint64_t T, uint32_t C) {
  const unsigned __int128 a = ((unsigned __int128)j << 32) + u;
  return (uint64_t)((a * T) / ((unsigned __int128)C << 32));
}

}  // namespace

int main() {
  const uint64_t TMAX = 1ull << 50;
  const uint32_t CMAX = FW_RSM_MAX_CHAINS;
  long bad_total = 0;

  long n = 0, bad = 0;
  for (int it = 0; it < 1500000; ++it) {
    uint32_t C = (uint32_t)(rnd() % CMAX) + 1;
    if (it % 7 == 0) C = 1u << (rnd() % 21);
    if (it % 11 == 0) C = CMAX;
    if (it % 13 == 0) C = (uint32_t)(rnd() % 64) + 1;
    const uint32_t j = (uint32_t)(rnd() % C), u = (uint32_t)rnd();
    uint64_t T = rnd() % TMAX + 1;
    if (it % 5 == 0) T = (uint64_t)C << 30;            // every chain at the heaviest weight
    if (it % 17 == 0) T = (1ull << 30) + rnd() % 1024;  // one heavy chain and a little dust
    ++n;
    bad += fw_rsm_point(j, u, T, C) != exact(j, u, T, C);
  }
  std::printf("random cases %ld mismatches %ld\n", n, bad);
  bad_total += bad;

  n = bad = 0;
  const uint32_t Cs[] = {1, 2, 3, 5, 63, 64, 65, 77, 65535, 65536, 65537, CMAX - 1, CMAX};
  const uint32_t us[] = {0, 1, 2, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFEu, 0xFFFFFFFFu};
  const uint64_t Ts[] = {1, 2, (1ull << 30) - 1, 1ull << 30, (1ull << 30) + 1, (1ull << 32) - 1,
                         1ull << 32, (1ull << 32) + 1, (1ull << 48) + 12345, TMAX - 1, TMAX};
  for (uint32_t C : Cs)
    for (uint32_t u : us)
      for (uint64_t T : Ts) {
        const uint32_t js[] = {0, 1, C / 2, C > 1 ? C - 2 : 0, C - 1};
        for (uint32_t j : js) {
          if (j >= C) continue;
          ++n;
          bad += fw_rsm_point(j, u, T, C) != exact(j, u, T, C);
        }
      }
  // and more values of T around every power of two
  for (int b = 0; b <= 50; ++b)
    for (int d = -1; d <= 1; ++d) {
      const uint64_t T = (1ull << b) + (uint64_t)(int64_t)d;
      if (T < 1 || T > TMAX) continue;
      for (uint32_t C : Cs)
        for (uint32_t u : us) {
          ++n;
          bad += fw_rsm_point(C - 1, u, T, C) != exact(C - 1, u, T, C);
        }
    }
  std::printf("extreme cases %ld mismatches %ld\n", n, bad);
  bad_total += bad;

  n = bad = 0;
  for (int it = 0; it < 40; ++it) {
    const uint32_t C = it < 2 ? CMAX >> 4 : (uint32_t)(rnd() % 8192) + 1, u = (uint32_t)rnd();
    const uint64_t T = it % 3 == 0 ? (uint64_t)C << 30 : rnd() % TMAX + 1;
    uint64_t prev = 0;
    for (uint32_t j = 0; j < C; ++j) {
      const uint64_t p = fw_rsm_point(j, u, T, C);
      ++n;
      bad += p < prev || p >= T || p != exact(j, u, T, C);
      prev = p;
    }
  }
  std::printf("ascending cases %ld mismatches %ld\n", n, bad);
  bad_total += bad;
  return bad_total ? 1 : 0;
}
