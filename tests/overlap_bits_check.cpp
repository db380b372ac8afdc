// overlap_bits_check.cpp — the field arithmetic of the plan-overlap kernel on the host.
//
// Includes flipcomplexityempirical_amd/csrc/fw_overlap_bits.h (the same text the kernel
// compiles) and compares, for each of the five label widths, the equality mask, the pair mask,
// the differing-fields mask, the field extraction and the tail mask with a per-field loop over
// the bit string.  Word groups: random words, words with few distinct labels (long runs, as in
// a plan), and pairs that differ only in the fields that straddle a dword (3 and 5 bits) or in
// single bits of them.  Prints one "name cases N mismatches M" line per check; exit status 1
// on any mismatch.
#include <stdint.h>
#include <stdio.h>

#include "../flipcomplexityempirical_amd/csrc/fw_overlap_bits.h"

namespace {

uint64_t rng_state = 0x9e3779b97f4a7c15ull;
uint64_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

// field j of an LB-dword group, bit by bit
template <int LB>
uint32_t field_loop(const uint32_t* w, int j) {
  uint32_t v = 0;
  for (int b = 0; b < LB; ++b) {
    const int bit = j * LB + b;
    v |= ((w[bit >> 5] >> (bit & 31)) & 1u) << b;
  }
  return v;
}

template <int LB>
void set_field(uint32_t* w, int j, uint32_t v) {
  for (int b = 0; b < LB; ++b) {
    const int bit = j * LB + b;
    w[bit >> 5] = (w[bit >> 5] & ~(1u << (bit & 31))) | (((v >> b) & 1u) << (bit & 31));
  }
}

template <int LB>
bool straddles(int j) {
  return ((j * LB) >> 5) != ((j * LB + LB - 1) >> 5);
}

struct Tally {
  long long cases = 0, bad = 0;
};

// every check of one pair of groups
template <int LB>
void check_pair(const uint32_t* r, const uint32_t* x, Tally* eq, Tally* pair, Tally* diff,
                Tally* field) {
  uint32_t fr[32], fx[32];
  for (int j = 0; j < 32; ++j) {
    fr[j] = field_loop<LB>(r, j);
    fx[j] = field_loop<LB>(x, j);
    field->cases += 2;
    field->bad += fw_ovl_field<LB>(r, j) != fr[j];
    field->bad += fw_ovl_field<LB>(x, j) != fx[j];
  }
  uint32_t want = 0;
  for (int j = 0; j < 32; ++j) want |= (uint32_t)(fr[j] != fx[j]) << j;
  diff->cases += 1;
  diff->bad += fw_ovl_diff_mask<LB>(r, x) != want;
  // the values that occur at three nodes, and one that may not occur
  const int at[3] = {(int)(rnd() & 31), (int)(rnd() & 31), 31};
  for (int t = 0; t < 4; ++t) {
    const uint32_t a = t < 3 ? fr[at[t]] : (uint32_t)(rnd() & ((1u << LB) - 1u));
    const uint32_t b = t < 3 ? fx[at[t]] : (uint32_t)(rnd() & ((1u << LB) - 1u));
    uint32_t we = 0, wp = 0;
    for (int j = 0; j < 32; ++j) {
      we |= (uint32_t)(fx[j] == b) << j;
      wp |= (uint32_t)(fr[j] == a && fx[j] == b) << j;
    }
    eq->cases += 1;
    eq->bad += fw_ovl_eq_mask<LB>(x, b) != we;
    pair->cases += 1;
    pair->bad += fw_ovl_pair_mask<LB>(r, x, a, b) != wp;
  }
}

template <int LB>
bool check_width() {
  Tally eq, pair, diff, field, strad;
  const long long rounds = 350000;  // x 3 kinds of groups: more than 10^6 per width
  for (long long it = 0; it < rounds; ++it) {
    uint32_t r[LB], x[LB];
    // random words
    for (int i = 0; i < LB; ++i) {
      r[i] = (uint32_t)rnd();
      x[i] = (uint32_t)rnd();
    }
    check_pair<LB>(r, x, &eq, &pair, &diff, &field);
    // few distinct labels in runs
    uint32_t lr = (uint32_t)rnd(), lx = (uint32_t)rnd();
    for (int j = 0; j < 32; ++j) {
      if ((rnd() & 7) == 0) lr = (uint32_t)rnd();
      if ((rnd() & 7) == 0) lx = (uint32_t)rnd();
      set_field<LB>(r, j, lr & ((1u << LB) - 1u));
      set_field<LB>(x, j, lx & ((1u << LB) - 1u));
    }
    check_pair<LB>(r, x, &eq, &pair, &diff, &field);
    // equal but for the straddling fields (aligned widths: but for one field), where a random
    // subset of the bits differs: a single bit on either side of the dword border included
    for (int i = 0; i < LB; ++i) x[i] = r[i];
    uint32_t want = 0;
    for (int j = 0; j < 32; ++j) {
      const bool pick = (LB == 3 || LB == 5) ? straddles<LB>(j) : j == (int)(it & 31);
      if (!pick) continue;
      const uint32_t flip = (it & 1) ? 1u << (rnd() % LB) : (uint32_t)(rnd() & ((1u << LB) - 1u));
      set_field<LB>(x, j, field_loop<LB>(r, j) ^ flip);
      want |= (uint32_t)(flip != 0) << j;
    }
    strad.cases += 1;
    strad.bad += fw_ovl_diff_mask<LB>(r, x) != want;
    check_pair<LB>(r, x, &eq, &pair, &diff, &field);
  }
  printf("eq%d cases %lld mismatches %lld\n", LB, eq.cases, eq.bad);
  printf("pair%d cases %lld mismatches %lld\n", LB, pair.cases, pair.bad);
  printf("diff%d cases %lld mismatches %lld\n", LB, diff.cases, diff.bad);
  printf("field%d cases %lld mismatches %lld\n", LB, field.cases, field.bad);
  printf("straddle%d cases %lld mismatches %lld\n", LB, strad.cases, strad.bad);
  return !(eq.bad || pair.bad || diff.bad || field.bad || strad.bad);
}

bool check_tail() {
  Tally t;
  for (int count = 1; count <= 32; ++count) {
    uint32_t want = 0;
    for (int j = 0; j < 32; ++j) want |= (uint32_t)(j < count) << j;
    t.cases += 1;
    t.bad += fw_ovl_tail_mask(count) != want;
  }
  printf("tail cases %lld mismatches %lld\n", t.cases, t.bad);
  return t.bad == 0;
}

}  // namespace

int main() {
  bool ok = check_tail();
  ok = check_width<2>() && ok;
  ok = check_width<3>() && ok;
  ok = check_width<4>() && ok;
  ok = check_width<5>() && ok;
  ok = check_width<8>() && ok;
  return ok ? 0 : 1;
}
