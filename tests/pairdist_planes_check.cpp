// pairdist_planes_check.cpp — the bit-plane arithmetic and the blocking plan of the pairwise plan
// distance (csrc/fw_pairdist_planes.h, csrc/fw_pairdist_plan.h) on the host, compiled from the
// same text as the kernel.  For every label width it transposes pairs of 32-node groups into
// planes and compares the XOR / OR / popcount count with a per-field loop, at every tail length
// 1..32: random words, runs of few labels, pairs that differ only in the fields that straddle a
// dword, and pairs that differ in one bit of such a field.  It also checks that a plane holds
// exactly bit p of every field, and that over n = 1 .. 5000 and every width and forced tile and
// chunk the plan's chunks cover every group exactly once and fit the LDS budget.
// Prints "<name><LB> cases <n> mismatches <m>" per check; exit status 1 on any mismatch.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../flipcomplexityempirical_amd/csrc/fw_pairdist_plan.h"
#include "../flipcomplexityempirical_amd/csrc/fw_pairdist_planes.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return (uint32_t)(rng_state >> 16);
}

template <int LB>
static uint32_t field(const uint32_t w[LB], int j) {
  uint32_t v = 0;
  for (int q = 0; q < LB; ++q) {
    const int bit = j * LB + q;
    v |= ((w[bit >> 5] >> (bit & 31)) & 1u) << q;
  }
  return v;
}

template <int LB>
static void set_field(uint32_t w[LB], int j, uint32_t v) {
  for (int q = 0; q < LB; ++q) {
    const int bit = j * LB + q;
    w[bit >> 5] = (w[bit >> 5] & ~(1u << (bit & 31))) | (((v >> q) & 1u) << (bit & 31));
  }
}

template <int LB>
static bool straddles(int j) {
  return ((j * LB) >> 5) != ((j * LB + LB - 1) >> 5);
}

// one pair of groups at every tail length: the plane count against the per-field loop, and the
// planes themselves against the fields' bits
template <int LB>
static void check_pair(const uint32_t a[LB], const uint32_t b[LB], long* cases, long* bad,
                       long* plane_cases, long* plane_bad) {
  for (int count = 1; count <= 32; ++count) {
    const uint32_t tail = fw_ovl_tail_mask(count);
    uint32_t pa[LB], pb[LB];
    fw_pwd_planes<LB>(a, tail, pa);
    fw_pwd_planes<LB>(b, tail, pb);
    uint32_t want = 0;
    for (int j = 0; j < count; ++j) want += field<LB>(a, j) != field<LB>(b, j);
    *bad += fw_pwd_count(fw_pwd_diff<LB>(pa, pb)) != want;
    *cases += 1;
    if (count == 32 || count == 13) {
      for (int q = 0; q < LB; ++q) {
        uint32_t plane = 0;
        for (int j = 0; j < count; ++j) plane |= ((field<LB>(a, j) >> q) & 1u) << j;
        *plane_bad += plane != pa[q];
        *plane_cases += 1;
      }
    }
  }
}

template <int LB>
static long check_width() {
  long cases = 0, bad = 0, pc = 0, pb = 0, sc = 0, sb = 0, rc = 0, rb = 0;
  uint32_t a[LB], b[LB];
  // random words; then b a copy of a with a few fields redrawn
  for (int t = 0; t < 6000; ++t) {
    for (int i = 0; i < LB; ++i) a[i] = rnd(), b[i] = rnd();
    check_pair<LB>(a, b, &cases, &bad, &pc, &pb);
    for (int i = 0; i < LB; ++i) b[i] = a[i];
    for (int r = rnd() % 5; r > 0; --r) set_field<LB>(b, (int)(rnd() % 32), rnd() & ((1u << LB) - 1u));
    check_pair<LB>(a, b, &cases, &bad, &pc, &pb);
  }
  // runs of few labels, as plans have them
  for (int t = 0; t < 6000; ++t) {
    for (int which = 0; which < 2; ++which) {
      uint32_t* w = which ? b : a;
      for (int i = 0; i < LB; ++i) w[i] = 0;
      uint32_t v = rnd() % 3;
      for (int j = 0; j < 32; ++j) {
        if (rnd() % 6 == 0) v = rnd() % (LB == 2 ? 4 : 5);
        set_field<LB>(w, j, v);
      }
    }
    check_pair<LB>(a, b, &rc, &rb, &pc, &pb);
  }
  // pairs that differ only in straddling fields (3 and 5 bits have them), in the whole field or
  // in one bit of it; the other widths take the fields next to a dword edge instead
  for (int t = 0; t < 400; ++t) {
    for (int i = 0; i < LB; ++i) a[i] = rnd();
    for (int j = 0; j < 32; ++j) {
      const bool edge = straddles<LB>(j) || (j * LB) % 32 == 0 || (j * LB + LB) % 32 == 0;
      if (!edge) continue;
      for (int i = 0; i < LB; ++i) b[i] = a[i];
      set_field<LB>(b, j, ~field<LB>(a, j) & ((1u << LB) - 1u));
      check_pair<LB>(a, b, &sc, &sb, &pc, &pb);
      for (int q = 0; q < LB; ++q) {
        for (int i = 0; i < LB; ++i) b[i] = a[i];
        set_field<LB>(b, j, field<LB>(a, j) ^ (1u << q));
        check_pair<LB>(a, b, &sc, &sb, &pc, &pb);
      }
    }
  }
  printf("count%d cases %ld mismatches %ld\n", LB, cases, bad);
  printf("runs%d cases %ld mismatches %ld\n", LB, rc, rb);
  printf("straddle%d cases %ld mismatches %ld\n", LB, sc, sb);
  printf("planes%d cases %ld mismatches %ld\n", LB, pc, pb);
  return bad + rb + sb + pb;
}

// every group in exactly one chunk, the image inside the budget, a thread's items within ipt
static long check_plans() {
  long cases = 0, bad = 0;
  const int widths[5] = {2, 3, 4, 5, 8}, tiles[4] = {0, 16, 32, 64}, chunks[5] = {-1, 1, 2, 3, 7};
  std::vector<int> seen;
  for (int n = 1; n <= 5000; ++n)
    for (int lb : widths)
      for (int tile : tiles)
        for (int chunk : chunks) {
          if (n > 300 && n % 37 && (tile || chunk > 0)) continue;  // forced plans on a subset
          const FwPwdPlan q = fw_pwd_plan(n, lb, tile, chunk);
          bool ok = q.n_groups == (n + 31) / 32 && q.chunk >= 1 && q.lds_bytes <= FW_PWD_LDS_BYTES &&
                    q.lds_bytes == 2 * q.chunk * lb * q.rs * 4 && q.rs % 4 == 0 &&
                    q.rs >= 2 * q.tile && (tile == 0 ? q.tile == FW_PWD_TILE : q.tile == tile) &&
                    2 * q.tile * q.chunk <= FW_PWD_THREADS * q.ipt && q.ipt * lb <= 16 &&
                    (q.tile / 4) * (q.tile / 4) <= FW_PWD_THREADS &&
                    (chunk < 1 || q.chunk <= chunk);
          seen.assign((size_t)q.n_groups, 0);
          for (int c = 0; c < q.n_chunks; ++c) {
            int g0, gn;
            fw_pwd_chunk_range(q, c, &g0, &gn);
            ok = ok && gn >= 1 && gn <= q.chunk;
            for (int g = g0; g < g0 + gn && g < q.n_groups; ++g) seen[(size_t)g] += 1;
            ok = ok && g0 + gn <= q.n_groups;
          }
          for (int s : seen) ok = ok && s == 1;
          bad += !ok;
          cases += 1;
        }
  printf("plan cases %ld mismatches %ld\n", cases, bad);
  return bad;
}

int main() {
  long bad = 0;
  bad += check_width<2>();
  bad += check_width<3>();
  bad += check_width<4>();
  bad += check_width<5>();
  bad += check_width<8>();
  bad += check_plans();
  return bad ? 1 : 0;
}
