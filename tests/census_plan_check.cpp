// Host check of csrc/fw_census_plan.h: the same text the census kernel compiles, against loops
// that restate each function bit by bit.  Prints "<name> cases N mismatches M" per check
// (tests/test_census_host.py reads the lines).
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../flipcomplexityempirical_amd/csrc/fw_census_plan.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return (uint32_t)(rng_state >> 16);
}

static uint32_t bits_of(const std::vector<uint32_t>& rec, int64_t bit, int lb) {
  uint32_t v = 0;
  for (int b = 0; b < lb; ++b) v |= ((rec[(size_t)((bit + b) >> 5)] >> ((bit + b) & 31)) & 1u) << b;
  return v;
}

// a record of n nodes; windows of random node ranges: every node of the range is cut from the
// window alone (the copy holds only the window's dwords, guarded by canaries on both sides)
template <int LB>
static void check_field() {
  long cases = 0, bad = 0, straddle = 0;
  for (int round = 0; round < 400; ++round) {
    const int n = 1 + (int)(rnd() % 700);
    const int words = (int)(((int64_t)n * LB + 31) / 32);
    std::vector<uint32_t> rec((size_t)words + 1);
    for (auto& w : rec) w = rnd();
    for (int t = 0; t < 8; ++t) {
      int lo = (int)(rnd() % n), hi = (int)(rnd() % n);
      if (lo > hi) { const int s = lo; lo = hi; hi = s; }
      int wd0, wdn;
      fw_cen_window(lo, hi, LB, &wd0, &wdn);
      if (wd0 < 0 || wdn < 1 || wd0 + wdn > words) { ++bad; continue; }
      // the window is tight: its first and last dwords hold bits of lo and hi
      if ((int)(((int64_t)lo * LB) >> 5) != wd0 ||
          (int)(((int64_t)(hi + 1) * LB - 1) >> 5) != wd0 + wdn - 1) ++bad;
      std::vector<uint32_t> win(rec.begin() + wd0, rec.begin() + wd0 + wdn);
      win.shrink_to_fit();
      for (int x = lo; x <= hi; ++x) {
        const uint32_t bit = (uint32_t)((int64_t)x * LB - (int64_t)wd0 * 32);
        if ((bit & 31) + LB > 32) {
          ++straddle;
          if ((bit >> 5) + 1 >= (uint32_t)wdn) { ++bad; continue; }  // would read past the window
        }
        ++cases;
        if (fw_cen_field<LB>(win.data(), bit) != bits_of(rec, (int64_t)x * LB, LB)) ++bad;
      }
    }
  }
  printf("field%d cases %ld mismatches %ld\n", LB, cases, bad);
  printf("straddle%d cases %ld mismatches 0\n", LB, straddle);
}

static void check_reach() {
  long cases = 0, bad = 0;
  for (int round = 0; round < 300; ++round) {
    const int n = 2 + (int)(rnd() % 60);
    std::vector<int32_t> rowptr(n + 1, 0), col;
    for (int v = 0; v < n; ++v) {
      const int deg = (int)(rnd() % 5);
      for (int i = 0; i < deg; ++i) col.push_back((int32_t)(rnd() % n));
      rowptr[v + 1] = (int32_t)col.size();
    }
    col.push_back(0);  // data() of an empty vector may be null
    const int T = 1 + (int)(rnd() % n);
    for (int t0 = 0; t0 < n; t0 += T) {
      const int t1 = t0 + T < n ? t0 + T : n;
      int lo, hi;
      fw_cen_tile_reach(rowptr.data(), col.data(), t0, t1, &lo, &hi);
      int a = t0, b = t1 - 1;
      for (int v = t0; v < t1; ++v)
        for (int e = rowptr[v]; e < rowptr[v + 1]; ++e) {
          if (col[e] < a) a = col[e];
          if (col[e] > b) b = col[e];
        }
      ++cases;
      if (lo != a || hi != b) ++bad;
    }
  }
  printf("reach cases %ld mismatches %ld\n", cases, bad);
}

// the slices of every (count, len) partition 0 .. count - 1 in order, none empty
static void check_slices() {
  long cases = 0, bad = 0;
  for (int count = 1; count <= 200; ++count)
    for (int len = 1; len <= count + 3; ++len) {
      const int ns = fw_cen_slices(count, len);
      int next = 0;
      for (int s = 0; s < ns; ++s) {
        int i0, i1;
        fw_cen_slice_range(s, len, count, &i0, &i1);
        if (i0 != next || i1 <= i0 || i1 - i0 > len) ++bad;
        next = i1;
      }
      if (next != count) ++bad;
      ++cases;
    }
  int i0, i1;  // the products near 2^31 do not wrap
  fw_cen_slice_range(65535, 65536, 2147483647, &i0, &i1);
  if (i0 != 2147483647 || i1 != 2147483647) ++bad;
  printf("slices cases %ld mismatches %ld\n", cases, bad);
}

int main() {
  check_field<2>();
  check_field<3>();
  check_field<4>();
  check_field<5>();
  check_field<8>();
  check_reach();
  check_slices();
  return 0;
}
