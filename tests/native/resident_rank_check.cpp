// Test harness (CPU): the arithmetic of the adjoint's step-resident contact tables that the kernel shares with the host (csrc/dc_launchplan.h) —
// the slot of a contact vertex as its rank among the set bits of the contact mask (adj_rank: per-word count + popcount below the bit) against a
// brute-force count, and the "fits / does not fit" rule of list + mask + counts + tables in the list's room (adj_tables_fit) against the layout
// the kernel derives from it.
//   g++ -O2 -std=c++17 -Wall -I diffcloth_amd/csrc tests/native/resident_rank_check.cpp -o resident_rank_check
// Prints one line per group of checks and exits non-zero on the first failure (driven by tests/test_resident_rank.py).
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>
#include "dc_launchplan.h"

using namespace dc;

static void fail(const std::string &what) { std::printf("FAIL %s\n", what.c_str()); std::exit(1); }
static void eq(long long got, long long want, const std::string &what) {
  if (got != want) fail(what + ": " + std::to_string(got) + ", expected " + std::to_string(want));
}

// mask and counts as k_adjoint_step builds them: bit i & 31 of word i >> 5, adj_mask_words(N) words (the last ones zero past N), and per word the
// number of set bits in all words before it
static void check_mask(const std::vector<char> &in, const std::string &tag) {
  const int N = (int) in.size(), mw = adj_mask_words(N);
  if (mw * 32 < N) fail(tag + ": mask words do not cover N");
  std::vector<unsigned> mask(mw, 0u), prefix(mw, 0u);
  for (int i = 0; i < N; i++) if (in[i]) mask[i >> 5] |= 1u << (i & 31);
  unsigned run = 0;
  for (int w = 0; w < mw; w++) { prefix[w] = run; run += (unsigned) __builtin_popcount(mask[w]); }
  int brute = 0;
  for (int i = 0; i < N; i++) {
    // (the rank is asked for set bits only, but the count below the bit is defined for every vertex)
    eq(adj_rank(mask.data(), prefix.data(), i), brute, tag + ": rank of vertex " + std::to_string(i));
    if (in[i]) brute++;
  }
  eq(run, brute, tag + ": total");
}

int main() {
  // ---- mask words: two per 64 vertices, rounded up ----
  eq(adj_mask_words(1), 2, "adj_mask_words(1)"); eq(adj_mask_words(64), 2, "adj_mask_words(64)"); eq(adj_mask_words(65), 4, "adj_mask_words(65)");
  eq(adj_mask_words(2304), 72, "adj_mask_words(2304)"); eq(adj_mask_words(10000), 314, "adj_mask_words(10000)");
  std::printf("ok mask words\n");

  // ---- ranks: set bits at 0, 31, 32 and N - 1; N not a multiple of 64; empty, full and random masks of several densities ----
  std::mt19937 rng(11);
  for (int N : {1, 31, 32, 33, 63, 64, 65, 100, 127, 129, 1000, 2304, 4097, 10000}) {
    std::vector<char> m(N, 0);
    check_mask(m, "empty N=" + std::to_string(N));
    for (int p : {0, 31, 32, N - 1}) if (p < N) m[p] = 1;
    check_mask(m, "edges N=" + std::to_string(N));
    for (int p : {0, 31, 32, N - 1}) {
      if (p >= N) continue;
      std::vector<char> one(N, 0);
      one[p] = 1;
      check_mask(one, "single bit " + std::to_string(p) + " N=" + std::to_string(N));
    }
    std::fill(m.begin(), m.end(), 1);
    check_mask(m, "full N=" + std::to_string(N));
    for (double dens : {0.01, 0.15, 0.5, 0.9}) {
      std::bernoulli_distribution bit(dens);
      for (int rep = 0; rep < 4; rep++) {
        for (int i = 0; i < N; i++) m[i] = bit(rng);
        if (rep & 1) { m[0] = 1; m[N - 1] = 1; if (N > 32) { m[31] = 1; m[32] = 1; } }
        check_mask(m, "random N=" + std::to_string(N) + " density " + std::to_string(dens));
      }
    }
  }
  std::printf("ok ranks\n");

  // ---- table sizes, by hand: header 4; 8 per self contact; 2 per working-set slot; layers + 1; 9 per primitive-contact vertex; to a multiple of 4 ----
  eq(adj_tables_floats(0, 0, 0, 0), 8, "tables(0, 0, 0, 0)");                      // 4 + 1 = 5 -> 8
  eq(adj_tables_floats(10, 0, 0, 0), 96, "tables(10, 0, 0, 0)");                   // 4 + 1 + 90 = 95 -> 96
  eq(adj_tables_floats(540, 1000, 500, 3), 10868, "tables(540, 1000, 500, 3)");    // 4 + 4000 + 2000 + 4 + 4860 = 10868
  std::printf("ok table sizes\n");

  // ---- the rule: fits <=> 3 (nplist + M) + 2 mask words + tables + 3 <= 3 ycap and tables <= cap. Against the layout the kernel derives: the
  //      tables start at the absolute float index (ybase + 3 ycap - 2 mw - tables) & ~3 and must not reach into the list, for every ybase ----
  std::uniform_int_distribution<int> un(1, 12000), uc(0, 3000), ul(0, 40), ub(0, 40000);
  long long fits = 0, refused = 0;
  for (int rep = 0; rep < 20000; rep++) {
    const int N = un(rng), np = uc(rng) % (N + 1), nc = uc(rng), M = nc ? std::min(2 * nc, 1 + uc(rng) % (2 * nc)) : 0, nl = nc ? 1 + ul(rng) : 0;
    const int mw = adj_mask_words(N), tab = adj_tables_floats(np, M, nc, nl), need = 3 * (np + M) + 2 * mw + tab + 3;
    const int ycap_min = (need + 2) / 3;
    for (int ycap : {ycap_min - 1, ycap_min, ycap_min + 1, ycap_min + 1000}) {
      if (ycap < 0) continue;
      const bool want = 3 * ycap >= need;
      if (adj_tables_fit(ycap, N, np, M, nc, nl, 0x7fffffff) != want) fail("fit rule at ycap " + std::to_string(ycap));
      if (adj_tables_fit(ycap, N, np, M, nc, nl, tab) != want) fail("fit rule with the cap at the tables' size");
      if (adj_tables_fit(ycap, N, np, M, nc, nl, tab - 1)) fail("tables beyond the cap accepted");
      if (adj_tables_fit(ycap, N, np, M, nc, nl, 0)) fail("tables accepted with none allowed");
      if (!want) { refused++; continue; }
      fits++;
      const int ybase = ub(rng);
      const int start = (ybase + 3 * ycap - 2 * mw - tab) & ~3, list_end = ybase + 3 * (np + M), counts = ybase + 3 * ycap - 2 * mw;
      if (start % 4) fail("tables not 16-byte aligned");
      if (start < list_end) fail("tables reach into the list");
      if (start + tab > counts) fail("tables reach into the counts");
    }
  }
  // the headline's figures (100 x 100 cloth: ~540 primitive contacts, 500 self contacts with a working set of ~1 000, 6 100 entries of room) fit;
  // a sheet lying on a plane (every vertex in contact) does not
  if (!adj_tables_fit(6100, 10000, 540, 1000, 500, 3, 0x7fffffff)) fail("the headline's tables must fit");
  if (adj_tables_fit(6100, 10000, 10000, 0, 0, 0, 0x7fffffff)) fail("a sheet on a plane must not fit");
  std::printf("ok fit rule (%lld accepted, %lld refused)\n", fits, refused);
  std::printf("ALL OK\n");
  return 0;
}
