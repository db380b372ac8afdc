// Host check of csrc/fw_coassign_plan.h: the same text the device compiles.  Prints lines
// "<name> cases <n> mismatches <m>" (tests/test_coassign_host.py reads them):
//   planes<lb>    random label matrices with 1..97 members: the field cut from a tile's window
//                 is the label, the plane words hold the fields' bits, pad bits are zero
//   together<lb>  members - popcount(diff) over the member words equals a per-member loop
//   onebit<lb>    the same for pairs of entries whose labels differ in one bit, in one member
//   plan          tiles, windows and chunks cover every entry and member word exactly once
//                 inside the LDS bound (n up to 5,000, sparse and dense lists, forced plans)
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <random>
#include <vector>

#include "../flipcomplexityempirical_amd/csrc/fw_coassign_plan.h"

static std::mt19937_64 rng(20240611);

static int rnd(int lo, int hi) { return lo + (int)(rng() % (uint64_t)(hi - lo + 1)); }

// a record of exactly ceil(n lb / 32) dwords: a read past the label words is a sanitizer error
static std::vector<uint32_t> pack(const std::vector<uint32_t>& lab, int lb) {
  const size_t n = lab.size();
  std::vector<uint32_t> w((n * lb + 31) / 32, 0u);
  for (size_t x = 0; x < n; ++x) {
    const uint64_t bit = (uint64_t)x * lb, v = (uint64_t)lab[x] << (bit & 31);
    w[bit >> 5] |= (uint32_t)v;
    if ((bit & 31) + lb > 32) w[(bit >> 5) + 1] |= (uint32_t)(v >> 32);
  }
  return w;
}

static std::vector<int32_t> pick_nodes(int n, int m) {
  std::vector<int32_t> all(n);
  for (int i = 0; i < n; ++i) all[i] = i;
  std::shuffle(all.begin(), all.end(), rng);
  all.resize(m);
  std::sort(all.begin(), all.end());
  return all;
}

template <int LB>
static void check_width() {
  long planes_n = 0, planes_bad = 0, tog_n = 0, tog_bad = 0, one_n = 0, one_bad = 0;
  for (int members = 1; members <= 97; ++members) {
    const int n = rnd(1, 300), m = rnd(1, std::min(n, 150));
    const int kmax = members % 3 == 0 ? 2 : (1 << LB);  // runs of few labels too
    std::vector<int32_t> nodes = pick_nodes(n, m);
    if (members % 5 == 0) nodes[0] = 0;  // stays ascending: the smallest becomes node 0
    if (members % 7 == 0) nodes[m - 1] = n - 1;
    std::vector<std::vector<uint32_t>> lab(members, std::vector<uint32_t>(n));
    std::vector<std::vector<uint32_t>> rec(members);
    for (int c = 0; c < members; ++c) {
      for (int x = 0; x < n; ++x) lab[c][x] = (uint32_t)rnd(0, kmax - 1);
      rec[c] = pack(lab[c], LB);
    }
    const int n_words = (members + 31) / 32;
    // planes[word][plane][entry], as the device lays them out
    std::vector<uint32_t> pl((size_t)n_words * LB * m, 0u);
    for (int t = 0; t < fw_coa_tiles(m); ++t) {
      int e0, en, wd0, wdn;
      fw_coa_tile_window(nodes.data(), m, t, LB, &e0, &en, &wd0, &wdn);
      for (int j = e0; j < e0 + en; ++j) {
        const uint32_t bit = (uint32_t)((int64_t)nodes[j] * LB - (int64_t)wd0 * 32);
        for (int w = 0; w < n_words; ++w) {
          uint32_t x[32];
          const int count = std::min(32, members - 32 * w);
          for (int i = 0; i < count; ++i) {
            x[i] = fw_cen_field<LB>(rec[32 * w + i].data() + wd0, bit);
            ++planes_n;
            if (x[i] != lab[32 * w + i][nodes[j]]) ++planes_bad;
            if ((int)(bit >> 5) >= wdn) ++planes_bad;  // the field starts inside the window
          }
          for (int b = 0; b < LB; ++b) {
            const uint32_t word = fw_coa_plane_word(x, count, b);
            pl[((size_t)w * LB + b) * m + j] = word;
            for (int i = 0; i < 32; ++i) {
              const uint32_t want = i < count ? (lab[32 * w + i][nodes[j]] >> b) & 1u : 0u;
              ++planes_n;
              if (((word >> i) & 1u) != want) ++planes_bad;
            }
          }
        }
      }
    }
    // together over the words against a loop over the members
    for (int rep = 0; rep < 400; ++rep) {
      const int i = rnd(0, m - 1), j = rnd(0, m - 1);
      uint32_t got = 0, want = 0;
      for (int w = 0; w < n_words; ++w) {
        uint32_t a[LB], b[LB];
        for (int q = 0; q < LB; ++q) {
          a[q] = pl[((size_t)w * LB + q) * m + i];
          b[q] = pl[((size_t)w * LB + q) * m + j];
        }
        got += fw_coa_together<LB>(a, b, std::min(32, members - 32 * w));
      }
      for (int c = 0; c < members; ++c) want += lab[c][nodes[i]] == lab[c][nodes[j]];
      ++tog_n;
      if (got != want) ++tog_bad;
    }
    // two entries equal in every member but one, where they differ in one bit
    for (int rep = 0; rep < 200; ++rep) {
      const int c = rnd(0, members - 1), q = rnd(0, LB - 1), w = c / 32;
      uint32_t got = 0;
      for (int ww = 0; ww < n_words; ++ww) {
        uint32_t a[LB], b[LB];
        for (int r = 0; r < LB; ++r) a[r] = b[r] = pl[((size_t)ww * LB + r) * m + rnd(0, m - 1)];
        if (ww == w) b[q] ^= 1u << (c & 31);
        got += fw_coa_together<LB>(a, b, std::min(32, members - 32 * ww));
      }
      ++one_n;
      if (got != (uint32_t)members - 1u) ++one_bad;
    }
  }
  printf("planes%d cases %ld mismatches %ld\n", LB, planes_n, planes_bad);
  printf("together%d cases %ld mismatches %ld\n", LB, tog_n, tog_bad);
  printf("onebit%d cases %ld mismatches %ld\n", LB, one_n, one_bad);
}

static long plan_n = 0, plan_bad = 0;

static void check_plan(int n, int m, int lb, int per_group, int force_tile, int force_chunk,
                       int allow_stage, bool dense) {
  ++plan_n;
  std::vector<int32_t> nodes;
  if (dense) {
    const int first = rnd(0, n - m);
    for (int j = 0; j < m; ++j) nodes.push_back(first + j);
  } else {
    nodes = pick_nodes(n, m);
  }
  bool bad = false;
  // transpose tiles: every entry in exactly one tile, its field inside the tile's window
  std::vector<int> seen(m, 0);
  int wd_max = 0;
  const int lab_words = (int)(((int64_t)n * lb + 31) / 32);
  for (int t = 0; t < fw_coa_tiles(m); ++t) {
    int e0, en, wd0, wdn;
    fw_coa_tile_window(nodes.data(), m, t, lb, &e0, &en, &wd0, &wdn);
    if (en < 1 || en > FW_COA_TT || wd0 < 0 || wd0 + wdn > lab_words) bad = true;
    for (int j = e0; j < e0 + en; ++j) {
      ++seen[j];
      const int64_t lo = (int64_t)nodes[j] * lb, hi = lo + lb - 1;
      if (lo < (int64_t)wd0 * 32 || hi >= (int64_t)(wd0 + wdn) * 32) bad = true;
    }
    wd_max = std::max(wd_max, wdn);
  }
  for (int j = 0; j < m; ++j) bad |= seen[j] != 1;
  int nw, stride;
  const int staged = fw_coa_stage(wd_max, allow_stage, &nw, &stride);
  if (staged) {
    bad |= !allow_stage || stride < wd_max || !(stride & 1);
    bad |= (int64_t)64 * nw * (stride + 1) * 4 > FW_COA_LDS_BYTES;
  }
  bad |= nw != 1 && nw != 2 && nw != 4;
  // member words: every word belongs to one wave slot of one workgroup
  const int slots = (per_group + 63) / 64, spw = (slots + nw - 1) / nw, n_words = (per_group + 31) / 32;
  std::vector<int> wseen(n_words, 0);
  for (int s = 0; s < spw; ++s)
    for (int wave = 0; wave < nw; ++wave)
      for (int h = 0; h < 2; ++h) {
        const int w = 2 * (s * nw + wave) + h;
        if (w < n_words) ++wseen[w];
      }
  for (int w = 0; w < n_words; ++w) bad |= wseen[w] != 1;
  // the product's chunks
  const FwCoaPlan q = fw_coa_plan(per_group, lb, force_tile, force_chunk);
  bad |= q.n_words != n_words || q.lds_bytes > FW_COA_LDS_BYTES || q.chunk < 1;
  bad |= (1 << q.shift) != 2 * q.tile || q.rs < 2 * q.tile || q.rs % 4;
  bad |= q.chunk * lb * 2 * q.tile > FW_COA_THREADS * FW_COA_CARRY;
  bad |= (force_tile == 16 || force_tile == 32 || force_tile == 64) ? q.tile != force_tile
                                                                      : q.tile != FW_COA_TILE;
  bad |= force_chunk >= 1 && q.chunk > force_chunk;
  std::fill(wseen.begin(), wseen.end(), 0);
  for (int c = 0; c < q.n_chunks; ++c) {
    int w0, wn;
    fw_coa_chunk_range(q, c, &w0, &wn);
    if (wn < 1 || wn > q.chunk) bad = true;
    for (int w = w0; w < w0 + wn && w < n_words; ++w) ++wseen[w];
    if (w0 + wn > n_words) bad = true;
  }
  for (int w = 0; w < n_words; ++w) bad |= wseen[w] != 1;
  if (bad) ++plan_bad;
}

int main() {
  check_width<2>();
  check_width<3>();
  check_width<4>();
  check_width<5>();
  check_width<8>();
  const int widths[5] = {2, 3, 4, 5, 8};
  for (int n = 1; n <= 5000; ++n)
    for (int lb : widths) {
      const bool dense = n % 2 == 0;
      const int m = n % 3 == 0 ? n : rnd(1, n);
      const int per_group = n % 11 == 0 ? rnd(1, 70000) : rnd(1, 300);
      const int ft = n % 4 == 0 ? 16 << rnd(0, 2) : -1, fc = n % 5 == 0 ? rnd(1, 3) : -1;
      check_plan(n, m, lb, per_group, ft, fc, n % 7 != 0, dense);
    }
  printf("plan cases %ld mismatches %ld\n", plan_n, plan_bad);
  return 0;
}
