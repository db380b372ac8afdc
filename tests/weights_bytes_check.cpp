// Host check of flipcomplexityempirical_amd/csrc/fw_weights_bytes.h against the per-node
// rule of the grid kernel's weights4<2, MODE> (a node's weight under the pairs proposal is
// the number of distinct foreign labels among its grid neighbours, under the cut-edge
// proposal its cut degree), restated here node by node.  The 16 row-lanes of a chain are an
// array; a lane's neighbours are the array's neighbours.  The chain's LDS slot is a byte
// buffer laid out as the plan does (16-byte guard | labels, n / 4 + 8 bytes rounded up to 16
// | group sums), with random bytes everywhere outside the labels, so a field that should be
// masked and is not shows up as a mismatch.  Every byte offset read must lie in
// [-1, slot bytes).  Built and run by tests/test_weights_bytes_host.py.
// Prints one "name cases mismatches" line per set; exit status 1 on any mismatch.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../flipcomplexityempirical_amd/csrc/fw_weights_bytes.h"

namespace {

constexpr int GUARD = 16;

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {  // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}

int round16(int x) { return (x + 15) / 16 * 16; }
int per16(int G) { return G <= 32 ? 2 : G <= 64 ? 4 : G <= 160 ? 10 : 16; }  // the plan's

struct Tally {
  long long cases = 0, bad = 0, oob = 0, lo_edge = 0, hi_edge = 0;
};

// weights4<2, MODE>'s per-node rule on the unpacked labels
void node_ref(const std::vector<uint8_t>& lab, int x, int W, int H, uint32_t& w_pairs, uint32_t& cd) {
  const int r = x / W, c = x % W;
  const uint32_t lx = lab[x];
  uint32_t bits = 0;
  cd = 0;
  if (r > 0) { bits |= 1u << lab[x - W]; cd += lab[x - W] != lx; }
  if (c > 0) { bits |= 1u << lab[x - 1]; cd += lab[x - 1] != lx; }
  if (c < W - 1) { bits |= 1u << lab[x + 1]; cd += lab[x + 1] != lx; }
  if (r < H - 1) { bits |= 1u << lab[x + W]; cd += lab[x + W] != lx; }
  w_pairs = (uint32_t)__builtin_popcount(bits & ~(1u << lx));
}

template <bool CUT, bool NEED_CD>
void check_grid(int W, int H, const std::vector<uint8_t>& lab, Tally& t) {
  const int n = W * H, G = (n + 63) / 64;
  const int lab_bytes = round16((n * 2 + 7) / 8 + 8);
  const int slot = round16(lab_bytes) + 4 * 8 * per16(G);
  std::vector<uint8_t> mem(GUARD + slot);
  for (auto& b : mem) b = (uint8_t)rnd();
  uint8_t* const base = mem.data() + GUARD;
  for (int i = 0; i < n / 4; ++i)
    base[i] = (uint8_t)(lab[4 * i] | (lab[4 * i + 1] << 2) | (lab[4 * i + 2] << 4) | (lab[4 * i + 3] << 6));
  // groups 0 .. G: the derive loop walks pairs of groups and may visit group G (all masked)
  for (int gi = 0; gi <= G; ++gi) {
    uint32_t O[16], U[16], Dn[16], E[16], mN[16], mU[16], mD[16], mL[16], mR[16];
    for (int q = 0; q < 16; ++q) {
      const int x0 = gi * 64 + q * 4, r0 = x0 / W, c0 = x0 % W;
      int off[4];
      wb_offsets(gi, q, r0, W, H, off[0], off[1], off[2], off[3]);
      for (int i = 0; i < 4; ++i)
        if (off[i] < -1 || off[i] >= slot) {
          ++t.oob;
          off[i] = 0;
        }
      t.lo_edge += off[3] == -1;
      t.hi_edge += off[3] >= n / 4;
      O[q] = wb_onehot(base[off[0]]);
      U[q] = wb_onehot(base[off[1]]);
      Dn[q] = wb_onehot(base[off[2]]);
      E[q] = wb_edge(base[off[3]], q);
      wb_masks(x0, r0, c0, W, H, n, mN[q], mU[q], mD[q], mL[q], mR[q]);
    }
    for (int q = 0; q < 16; ++q) {
      uint32_t w4, cd4;
      wb_weights<CUT, NEED_CD>(O[q], U[q], Dn[q], q > 0 ? O[q - 1] : E[q], q < 15 ? O[q + 1] : E[q],
                               mN[q], mU[q], mD[q], mL[q], mR[q], w4, cd4);
      for (int tt = 0; tt < 4; ++tt) {
        const int x = gi * 64 + q * 4 + tt;
        uint32_t wp = 0, cd = 0;
        if (x < n) node_ref(lab, x, W, H, wp, cd);
        const uint32_t w_ref = CUT ? cd : wp;
        ++t.cases;
        if (((w4 >> (8 * tt)) & 0xFFu) != w_ref) ++t.bad;
        if ((NEED_CD || CUT) && ((cd4 >> (8 * tt)) & 0xFFu) != cd) ++t.bad;
      }
    }
  }
}

void fill_labels(std::vector<uint8_t>& lab, int W, int k, bool biased) {
  for (size_t x = 0; x < lab.size(); ++x) {
    uint8_t l = (uint8_t)(rnd() % (uint32_t)k);
    if (biased && x > 0) {
      // mostly the left or the upper neighbour's label: long runs, few cut edges
      const uint32_t r = rnd() % 16u;
      if (r < 8) l = lab[x - 1];
      else if (r < 14 && x >= (size_t)W) l = lab[x - W];
    }
    lab[x] = l;
  }
}

}  // namespace

int main() {
  Tally pairs, pairs_cd, cut;
  long long grids = 0;
  for (int W = 4; W <= 40; W += 4)
    for (int H = 1; H <= 40; ++H)
      for (int k = 2; k <= 4; ++k)
        for (int biased = 0; biased < 2; ++biased)
          for (int rep = 0; rep < 2; ++rep) {
            std::vector<uint8_t> lab((size_t)W * H);
            fill_labels(lab, W, k, biased != 0);
            check_grid<false, false>(W, H, lab, pairs);    // level 2, pairs proposal
            check_grid<false, true>(W, H, lab, pairs_cd);  // the derive loop (NEED_CD)
            check_grid<true, false>(W, H, lab, cut);       // cut-edge proposal (either call)
            ++grids;
          }
  const Tally* ts[3] = {&pairs, &pairs_cd, &cut};
  const char* names[3] = {"pairs", "pairs_cd", "cutedge"};
  long long bad = 0;
  for (int i = 0; i < 3; ++i) {
    printf("%s cases %lld mismatches %lld out_of_slot %lld (edge reads: %lld at -1, %lld past the labels)\n",
           names[i], ts[i]->cases, ts[i]->bad, ts[i]->oob, ts[i]->lo_edge, ts[i]->hi_edge);
    bad += ts[i]->bad + ts[i]->oob;
  }
  // wb_perm's host form against the selector's meaning, every selector byte 0..7
  long long pbad = 0, pn = 0;
  for (int it = 0; it < 100000; ++it) {
    const uint32_t hi = rnd(), lo = rnd(), sel = rnd() & 0x07070707u;
    const uint8_t src[8] = {(uint8_t)lo, (uint8_t)(lo >> 8), (uint8_t)(lo >> 16), (uint8_t)(lo >> 24),
                            (uint8_t)hi, (uint8_t)(hi >> 8), (uint8_t)(hi >> 16), (uint8_t)(hi >> 24)};
    const uint32_t r = wb_perm(hi, lo, sel);
    for (int i = 0; i < 4; ++i, ++pn) pbad += ((r >> (8 * i)) & 0xFFu) != src[(sel >> (8 * i)) & 7u];
  }
  printf("perm cases %lld mismatches %lld\n", pn, pbad);
  printf("grids %lld\n", grids);
  return bad + pbad ? 1 : 0;
}
