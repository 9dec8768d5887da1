// Property check of cal::shard_windows (calico_amd/csrc/shard.hpp, host only) on random and hand-picked count vectors:
// zeros, one dominant segment, a total of zero, nseg = 0 and 1, every world from 1 to 2 nseg + 1.
//
// With prefix(s) = counts[0] + ... + counts[s - 1] and b = shard_windows(counts, world):
//  1. b has world + 1 entries, b[0] = 0, b[world] = nseg, non-decreasing;
//  2. the blocks of the windows [b[r], b[r + 1]) sum to the total (every segment has exactly one owner);
//  3. cut r is the FIRST segment boundary at which the running count reaches r / world of the total:
//     prefix(b[r]) * world >= total * r, and prefix(s) * world < total * r for every s < b[r];
//  4. every prefix is within one segment's count of its share: 0 <= prefix(b[r]) - total r / world < counts[b[r] - 1]
//     (b[r] > 0; a cut at 0 needs a share of 0);
//  5. empty windows: none when no segment holds more than 1 / world of the blocks (and there are blocks); at least one when
//     there are more ranks than segments with blocks.
// Exits 0 and prints "OK <cases>" when all hold; prints the first violation and exits 1 otherwise.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../../calico_amd/csrc/shard.hpp"

namespace {

int64_t g_cases = 0;

bool fail(const char* what, const std::vector<int64_t>& c, int world, const std::vector<int>& b) {
  std::printf("FAILED: %s\n  world %d, counts:", what, world);
  for (int64_t v : c) std::printf(" %lld", (long long)v);
  std::printf("\n  boundaries:");
  for (int v : b) std::printf(" %d", v);
  std::printf("\n");
  return false;
}

bool check(const std::vector<int64_t>& c, int world) {
  ++g_cases;
  const int nseg = int(c.size());
  const std::vector<int> b = cal::shard_windows(c, world);
  std::vector<int64_t> prefix(size_t(nseg) + 1, 0);
  for (int s = 0; s < nseg; ++s) prefix[size_t(s) + 1] = prefix[size_t(s)] + c[size_t(s)];
  const int64_t total = prefix[size_t(nseg)];
  if (int(b.size()) != world + 1) return fail("world + 1 boundaries", c, world, b);
  if (b.front() != 0 || b.back() != nseg) return fail("boundaries start at 0 and end at nseg", c, world, b);
  int64_t owned = 0;
  int empty = 0;
  for (int r = 0; r < world; ++r) {
    if (b[size_t(r)] > b[size_t(r) + 1]) return fail("boundaries are non-decreasing", c, world, b);
    if (b[size_t(r)] < 0 || b[size_t(r) + 1] > nseg) return fail("boundaries inside [0, nseg]", c, world, b);
    const int64_t mine = prefix[size_t(b[size_t(r) + 1])] - prefix[size_t(b[size_t(r)])];
    owned += mine;
    empty += mine == 0 ? 1 : 0;
  }
  if (owned != total) return fail("the windows' blocks sum to the total", c, world, b);
  for (int r = 1; r < world; ++r) {
    const int cut = b[size_t(r)];
    const int64_t at = prefix[size_t(cut)];
    if (at * world < total * r) return fail("the running count at cut r reaches r / world of the total", c, world, b);
    for (int s = 0; s < cut; ++s)
      if (prefix[size_t(s)] * world >= total * r) return fail("cut r is the first such boundary", c, world, b);
    // within one segment's count of the share: (at - total r / world) < counts[cut - 1], in integers
    if (cut > 0 && !(at * world - total * r < c[size_t(cut) - 1] * world)) return fail("prefix within one segment of its share", c, world, b);
    if (cut == 0 && total * r != 0) return fail("a cut at 0 needs a share of 0", c, world, b);
  }
  // empty windows. No segment above total / world: prefix(b[r]) < total r / world + total / world <= prefix(b[r + 1]), so every
  // window owns something. More ranks than segments with blocks: some window owns nothing.
  {
    int64_t biggest = 0;
    for (int64_t v : c) biggest = v > biggest ? v : biggest;
    if (total > 0 && biggest * world <= total && empty != 0) return fail("no segment above 1 / world of the blocks, yet an empty window", c, world, b);
    int nonzero = 0;
    for (int64_t v : c) nonzero += v > 0 ? 1 : 0;
    if (world > nonzero && world > 1 && empty == 0) return fail("more ranks than segments with blocks, yet no empty window", c, world, b);
  }
  return true;
}

bool check_all_worlds(const std::vector<int64_t>& c) {
  const int nseg = int(c.size());
  for (int world = 1; world <= 2 * nseg + 1; ++world)
    if (!check(c, world)) return false;
  return true;
}

}  // namespace

int main() {
  // hand-picked: no segments, one segment, a total of zero, one dominant segment at either end and in the middle
  const std::vector<std::vector<int64_t>> fixed = {
      {}, {0}, {7}, {0, 0}, {0, 0, 0, 0, 0}, {5, 0}, {0, 5}, {1, 1}, {1000, 1, 1, 1}, {1, 1, 1, 1000}, {1, 1, 1000, 1, 1},
      {0, 0, 9, 0, 0}, {3, 3, 3, 3, 3, 3}, {104, 102}, {104, 114, 110, 112, 102}, {1, 0, 1, 0, 1, 0, 1},
      {int64_t(1) << 40, 1, int64_t(1) << 40},
  };
  for (const std::vector<int64_t>& c : fixed)
    if (!check_all_worlds(c)) return 1;
  {   // the exact windows of two small cases, by hand
    const std::vector<int> b = cal::shard_windows({104, 114, 110, 112, 102}, 5);      // total 542: shares at 108.4, 216.8, 325.2, 433.6
    if (b != std::vector<int>({0, 2, 2, 3, 4, 5})) { fail("hand-computed windows (rank 1 empty)", {104, 114, 110, 112, 102}, 5, b); return 1; }
    const std::vector<int> b2 = cal::shard_windows({104, 102}, 3);                    // shares at 68.7, 137.3
    if (b2 != std::vector<int>({0, 1, 2, 2})) { fail("hand-computed windows (last rank empty)", {104, 102}, 3, b2); return 1; }
  }
  std::mt19937_64 rng(20240607);
  for (int trial = 0; trial < 3000; ++trial) {
    const int nseg = int(rng() % 24);
    const int kind = int(rng() % 5);
    std::vector<int64_t> c(size_t(nseg), 0);
    for (int64_t& v : c) {
      switch (kind) {
        case 0: v = int64_t(rng() % 200); break;                          // plain
        case 1: v = (rng() % 3) ? 0 : int64_t(rng() % 50); break;         // mostly zeros
        case 2: v = int64_t(rng() % 4); break;                            // tiny counts, many ties
        case 3: v = 0; break;                                             // a total of zero
        default: v = int64_t(rng() % 10); break;                          // (a dominant segment is added below)
      }
    }
    if (kind == 4 && nseg > 0) c[size_t(rng() % uint64_t(nseg))] = 1000 + int64_t(rng() % 100000);
    if (!check_all_worlds(c)) return 1;
  }
  std::printf("OK %lld\n", (long long)g_cases);
  return 0;
}
