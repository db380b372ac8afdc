// Host check of flipcomplexityempirical_amd/csrc/fw_window_rows.h against the oracle's
// orc_window_verdict (oracle/flipchain_oracle.c, mask bit i * 7 + j, v = bit 24).  The seven
// row-lanes of a chain are an array here; a lane's neighbours are the array's neighbours.
// Built and run by tests/test_window_rows_host.py (link with the oracle's object file).
// Prints one "name masks mismatches" line per set; exit status 1 on any mismatch.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "../flipcomplexityempirical_amd/csrc/fw_window_rows.h"

extern "C" int orc_window_verdict(uint64_t A);

namespace {

constexpr uint64_t SRC_BITS = (1ull << 17) | (1ull << 23) | (1ull << 25) | (1ull << 31);
constexpr uint64_t ALL48 = ((1ull << 49) - 1) & ~(1ull << 24);

uint32_t amb_of(uint64_t A) {  // up, left, right, down
  return (uint32_t)(((A >> 17) & 1) | (((A >> 23) & 1) << 1) | (((A >> 25) & 1) << 2) |
                    (((A >> 31) & 1) << 3));
}

// the kernel's steps on seven lanes; rows[q]: the a-mask of window row q (7 bits)
int rows_verdict(const uint32_t rows[7], uint32_t amb, int* trips_out = nullptr) {
  uint32_t A4[7], x[7], y[7];
  for (int q = 0; q < 7; ++q) {
    A4[q] = rows[q] * 0x01010101u;
    x[q] = win_seed(q, amb) & A4[q];
  }
  int trips = 0;
  for (;;) {
    bool moving = false;
    for (int q = 0; q < 7; ++q)
      y[q] = win_dilate(x[q], q > 0 ? x[q - 1] : 0u, q < 6 ? x[q + 1] : 0u, A4[q]);
    for (int q = 0; q < 7; ++q) {
      x[q] = win_dilate(y[q], q > 0 ? y[q - 1] : 0u, q < 6 ? y[q + 1] : 0u, A4[q]);
      moving |= x[q] != y[q];
    }
    ++trips;
    if (!moving) break;
  }
  if (trips_out) *trips_out = trips;
  const uint32_t ex4 = win_exist4(amb);
  uint32_t vt = 0;
  for (int q = 0; q < 7; ++q) vt |= win_touch(x[q], q) | (win_miss(x[q], ex4) ? 1u : 0u);
  return win_verdict((vt & 1u) != 0u, vt, ex4);
}

int mask_verdict(uint64_t A) {
  uint32_t rows[7];
  for (int q = 0; q < 7; ++q) rows[q] = (uint32_t)(A >> (7 * q)) & 0x7Fu;
  return rows_verdict(rows, amb_of(A));
}

struct Tally {
  const char* name;
  uint64_t n = 0, bad = 0;
  uint64_t seen[3] = {0, 0, 0};  // verdicts -1, 0, 1 of the oracle
  void check(uint64_t A) {
    if (!(A & SRC_BITS)) return;  // no source: the window is never asked
    const int want = orc_window_verdict(A), got = mask_verdict(A);
    ++n;
    ++seen[want + 1];
    if (want != got) {
      if (bad < 5) std::fprintf(stderr, "%s: mask %012llx oracle %d rows %d\n", name,
                                (unsigned long long)A, want, got);
      ++bad;
    }
  }
  void add(const Tally& t) {
    n += t.n;
    bad += t.bad;
    for (int i = 0; i < 3; ++i) seen[i] += t.seen[i];
  }
  bool report() const {
    std::printf("%s masks %llu mismatches %llu (oracle: %llu undecided, %llu open, %llu joined)\n",
                name, (unsigned long long)n, (unsigned long long)bad, (unsigned long long)seen[0],
                (unsigned long long)seen[1], (unsigned long long)seen[2]);
    return bad == 0 && n > 0;
  }
};

uint64_t splitmix(uint64_t& s) {
  uint64_t z = (s += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// bits of `idx` scattered onto the set bits of `cells` (lowest first)
uint64_t scatter(uint64_t idx, uint64_t cells) {
  uint64_t out = 0;
  for (uint64_t c = cells; c; c &= c - 1, idx >>= 1)
    if (idx & 1) out |= c & (~c + 1);
  return out;
}

uint64_t cell(int i, int j) { return 1ull << (i * 7 + j); }

template <class F>
Tally parallel(const char* name, uint64_t count, F f) {
  unsigned nt = std::thread::hardware_concurrency();
  nt = nt < 1 ? 1 : (nt > 8 ? 8 : nt);
  std::vector<Tally> part(nt);
  std::vector<std::thread> th;
  for (unsigned t = 0; t < nt; ++t) {
    part[t].name = name;
    th.emplace_back([&, t] {
      for (uint64_t i = count * t / nt; i < count * (t + 1) / nt; ++i) part[t].check(f(i));
    });
  }
  Tally all;
  all.name = name;
  for (unsigned t = 0; t < nt; ++t) {
    th[t].join();
    all.add(part[t]);
  }
  return all;
}

// ---- the sets
// 1. every mask inside the central 5x5 (24 cells: every source subset with every surround)
Tally central5() {
  uint64_t cells = 0;
  for (int i = 1; i <= 5; ++i)
    for (int j = 1; j <= 5; ++j)
      if (i != 3 || j != 3) cells |= cell(i, j);
  return parallel("central5x5", 1ull << 24, [cells](uint64_t i) { return scatter(i, cells); });
}

// 2. sparse families: every subset of a fixed shape, together with each source subset
Tally families() {
  Tally t;
  t.name = "families";
  std::vector<uint64_t> shapes;
  uint64_t ring1 = 0, ring2 = 0, ring3 = 0;
  for (int i = 0; i < 7; ++i)
    for (int j = 0; j < 7; ++j) {
      const int d = std::max(std::abs(i - 3), std::abs(j - 3));
      if (d == 1) ring1 |= cell(i, j);
      if (d == 2) ring2 |= cell(i, j);
      if (d == 3) ring3 |= cell(i, j);
    }
  shapes.push_back(ring2);  // 16 cells
  uint64_t mid3 = 0;  // the three middle cells of every border side
  for (int t = 2; t <= 4; ++t) mid3 |= cell(0, t) | cell(6, t) | cell(t, 0) | cell(t, 6);
  shapes.push_back(ring3 & mid3);  // 12 cells
  // a one-cell-wide spiral arm: ring 2 opened beside the upper (left) source's cell, its far
  // end led out to the border; both senses
  const uint64_t s1 = (ring2 & ~cell(1, 2)) | cell(0, 1), s2 = (ring2 & ~cell(2, 1)) | cell(1, 0);
  shapes.push_back(s1);
  shapes.push_back(s2);
  // corridors from each source straight to its border side, plus the ring that may join them
  for (int side = 0; side < 4; ++side) {
    uint64_t c = ring1 & ~SRC_BITS;
    for (int s = 0; s < 3; ++s) {
      const int i = side == 0 ? s : side == 3 ? 6 - s : 3, j = side == 1 ? s : side == 2 ? 6 - s : 3;
      c |= cell(i, j);
      if (side == 0 || side == 3) c |= cell(i, 2) | cell(i, 4);
      else c |= cell(2, j) | cell(4, j);
    }
    shapes.push_back(c & ~SRC_BITS & ALL48);
  }
  for (uint64_t shape : shapes) {
    shape &= ~SRC_BITS;
    const int nb = __builtin_popcountll(shape);
    for (uint64_t s = 1; s < 16; ++s) {
      const uint64_t src = scatter(s, SRC_BITS);
      // subsets of the shape alone and on a filled ring-1 background
      for (uint64_t i = 0; i < (1ull << nb); ++i) {
        const uint64_t m = scatter(i, shape);
        t.check(m | src);
        if (!(shape & ring1)) t.check(m | src | (ring1 & ~SRC_BITS & (i * 0x9E3779B97F4A7C15ull >> 40)));
      }
    }
  }
  return t;
}

// 3. random 48-bit masks at three densities
Tally randoms() {
  Tally all;
  all.name = "random";
  const int thr[3] = {77, 128, 179};  // of 256: densities 0.3, 0.5, 0.7
  for (int d = 0; d < 3; ++d) {
    uint64_t s = 0xF11F0000ull + (uint64_t)d;
    for (int it = 0; it < 600000; ++it) {
      uint64_t A = 0;
      for (int w = 0; w < 7; ++w) {
        uint64_t r = splitmix(s);
        for (int b = 0; b < 7; ++b, r >>= 8)
          if ((int)(r & 255) < thr[d]) A |= 1ull << (w * 7 + b);
      }
      all.check(A & ALL48);
    }
  }
  return all;
}

// 4. rows and columns cut off (grid edges and corners, grids narrower or lower than 7)
Tally clipped() {
  Tally all;
  all.name = "clipped";
  uint64_t s = 0xC11BBEDull;
  for (int top = 0; top <= 3; ++top)
    for (int bot = 0; bot <= 3; ++bot)
      for (int lf = 0; lf <= 3; ++lf)
        for (int rt = 0; rt <= 3; ++rt) {
          uint64_t keep = 0;
          for (int i = top; i < 7 - bot; ++i)
            for (int j = lf; j < 7 - rt; ++j) keep |= cell(i, j);
          keep &= ALL48;
          for (int it = 0; it < 1500; ++it) {
            const uint64_t r1 = splitmix(s), r2 = splitmix(s);
            all.check(r1 & keep);
            all.check((r1 | r2) & keep);
            all.check(keep & ~(r1 & r2 & splitmix(s)));
          }
          all.check(keep);
        }
  return all;
}

// 5. the row mask against a per-cell loop: every bit offset, every a, labels at random
template <int LB>
bool row_masks() {
  uint64_t s = 0xABCD0000ull + LB, bad = 0, n = 0;
  for (uint32_t sh = 0; sh < 32; ++sh)
    for (int it = 0; it < 2000; ++it) {
      const uint64_t both = it == 0 ? 0ull : it == 1 ? ~0ull : splitmix(s);
      const uint32_t lo = (uint32_t)both, hi = (uint32_t)(both >> 32);
      for (uint32_t a = 0; a < (1u << LB); ++a) {
        uint32_t want = 0;
        for (int c = 0; c < 7; ++c)
          if (((both >> (sh + (uint32_t)(c * LB))) & ((1u << LB) - 1u)) == a) want |= 1u << c;
        bad += want != win_row_mask<LB>(lo, hi, sh, a);
        ++n;
      }
    }
  std::printf("row_mask%d cases %llu mismatches %llu\n", LB, (unsigned long long)n,
              (unsigned long long)bad);
  return bad == 0;
}

bool col_masks() {
  uint64_t bad = 0, n = 0;
  for (int W = 1; W <= 12; ++W)
    for (int vc = 0; vc < W; ++vc) {
      uint32_t want = 0;
      for (int c = 0; c < 7; ++c)
        if (vc - 3 + c >= 0 && vc - 3 + c < W) want |= 1u << c;
      bad += want != win_col_mask(vc, W);
      ++n;
    }
  std::printf("col_mask cases %llu mismatches %llu\n", (unsigned long long)n, (unsigned long long)bad);
  return bad == 0;
}

}  // namespace

int main() {
  bool ok = true;
  ok &= central5().report();
  ok &= families().report();
  ok &= randoms().report();
  ok &= clipped().report();
  ok &= row_masks<2>();
  ok &= row_masks<3>();
  ok &= row_masks<4>();
  ok &= col_masks();
  std::printf(ok ? "ok\n" : "FAILED\n");
  return ok ? 0 : 1;
}
