// Stand-alone check of the engine's free list (csrc/oi_arena.h), built with
// g++ -fsanitize=address,undefined (`make -C optimalinterpolation_amd
// arena_check`) and run by tests/test_arena.py.  No HIP, no GPU.
//
// Seeded random sequences of alloc / release run against a granule bitmap: one
// flag per 256-byte granule of the arena, set while a live block covers it.
// After every step
//   * the offset alloc returned is 256-aligned and is the lowest one at which
//     the bitmap has room (SIZE_MAX exactly when it has none),
//   * the new block overlaps no live block,
//   * the free list is sorted, disjoint, coalesced, inside the arena, and free
//     exactly where the bitmap is clear: free bytes = size - live bytes,
//   * a zero-byte alloc succeeds (in a full arena too) and neither it nor its
//     release changes the list,
//   * a release of SIZE_MAX, of a range outside the arena or of a block
//     already released changes nothing,
// and once everything is released the list is one block of the full size and a
// full-size alloc succeeds.  Named cases hold the literal sequences of defects
// found in the field.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "oi_arena.h"

namespace {

constexpr size_t G = 256;
int g_checks = 0;

[[noreturn]] void die(const std::string& where, const std::string& what) {
  std::printf("FAIL %s: %s\n", where.c_str(), what.c_str());
  std::exit(1);
}
#define REQUIRE(cond, where)                                      \
  do {                                                            \
    ++g_checks;                                                   \
    if (!(cond)) die(where, std::string(#cond) + " (line " + std::to_string(__LINE__) + ")"); \
  } while (0)

struct Live {
  size_t off, bytes;  // bytes as asked for (not rounded)
};

// The model beside the list under test.
struct Model {
  size_t size = 0;
  std::vector<char> used;  // per whole granule of [0, size)
  std::vector<Live> live;
  size_t live_bytes = 0;   // rounded

  void reset(size_t bytes) {
    size = bytes;
    used.assign(bytes / G, 0);
    live.clear();
    live_bytes = 0;
  }
  static size_t gran(size_t bytes) { return (bytes + G - 1) / G; }
  // lowest offset with `bytes` free, or SIZE_MAX
  size_t first_fit(size_t bytes) const {
    const size_t need = gran(bytes);
    size_t run = 0;
    for (size_t g = 0; g < used.size(); ++g) {
      run = used[g] ? 0 : run + 1;
      if (run == need) return (g + 1 - need) * G;
    }
    return SIZE_MAX;
  }
  void mark(size_t off, size_t bytes, char v, const std::string& where) {
    for (size_t g = off / G; g < off / G + gran(bytes); ++g) {
      REQUIRE(g < used.size(), where);
      REQUIRE(used[g] != v, where);  // no overlap with a live block / no double release
      used[g] = v;
    }
    if (v)
      live_bytes += gran(bytes) * G;
    else
      live_bytes -= gran(bytes) * G;
  }
};

// The list's invariants, and its agreement with the bitmap.
void check_state(const OiFreeList& fl, const Model& m, const std::string& where) {
  REQUIRE(fl.size() == m.size, where);
  size_t end_prev = 0, total = 0, largest = 0;
  bool first = true;
  std::vector<char> is_free(m.used.size(), 0);
  for (const auto& kv : fl.blocks()) {
    const size_t off = kv.first, len = kv.second;
    REQUIRE(len > 0, where);                       // no empty entries left behind
    REQUIRE(off % G == 0, where);
    REQUIRE(off < m.size && len <= m.size - off, where);
    REQUIRE(first || off > end_prev, where);       // disjoint and coalesced (never adjacent)
    REQUIRE(len % G == 0 || off + len == m.size, where);  // only the arena's tail may be ragged
    for (size_t g = off / G; g < (off + len) / G; ++g) is_free[g] = 1;
    end_prev = off + len;
    total += len;
    largest = len > largest ? len : largest;
    first = false;
  }
  for (size_t g = 0; g < m.used.size(); ++g) REQUIRE(is_free[g] == !m.used[g], where);
  REQUIRE(total == m.size - m.live_bytes, where);
  REQUIRE(fl.free_bytes() == total, where);
  REQUIRE(fl.largest_free() == largest, where);
}

size_t do_alloc(OiFreeList& fl, Model& m, size_t bytes, const std::string& where) {
  const auto before = fl.blocks();
  const size_t off = fl.alloc(bytes);
  if (bytes == 0) {
    REQUIRE(off != SIZE_MAX, where);  // an empty block needs no room
    REQUIRE(off <= m.size, where);
    REQUIRE(fl.blocks() == before, where);
    return off;
  }
  const size_t want = m.first_fit(bytes);
  REQUIRE(off == want, where);
  if (off == SIZE_MAX) {
    REQUIRE(fl.blocks() == before, where);
    return off;
  }
  REQUIRE(off % G == 0, where);
  m.mark(off, bytes, 1, where);
  m.live.push_back({off, bytes});
  check_state(fl, m, where);
  return off;
}

void do_release(OiFreeList& fl, Model& m, size_t idx, const std::string& where) {
  const Live b = m.live[idx];
  m.live[idx] = m.live.back();
  m.live.pop_back();
  fl.release(b.off, b.bytes);
  m.mark(b.off, b.bytes, 0, where);
  check_state(fl, m, where);
}

// releases that must change nothing
void bogus_releases(OiFreeList& fl, const Model& m, std::mt19937_64& rng, const std::string& where) {
  const auto before = fl.blocks();
  fl.release(SIZE_MAX, 0);
  fl.release(SIZE_MAX, 4096);
  fl.release(SIZE_MAX, SIZE_MAX);
  fl.release(m.size, 256);
  fl.release(m.size + 256, 1);
  fl.release(0, m.size + 1);
  fl.release(0, SIZE_MAX);
  fl.release(256, SIZE_MAX - 100);
  if (m.size >= 512) fl.release(m.size - 256, 257);
  for (const Live& b : m.live) fl.release(b.off, 0);  // the empty block at a live offset
  fl.release(rng() % (m.size + 1), 0);
  REQUIRE(fl.blocks() == before, where);
}

void release_all_and_check(OiFreeList& fl, Model& m, std::mt19937_64& rng, const std::string& where) {
  while (!m.live.empty()) do_release(fl, m, rng() % m.live.size(), where);
  REQUIRE(fl.blocks().size() == 1, where);
  REQUIRE(fl.blocks().begin()->first == 0 && fl.blocks().begin()->second == m.size, where);
  const size_t whole = m.size / G * G;
  REQUIRE(do_alloc(fl, m, whole, where) == 0, where);
  do_release(fl, m, 0, where);
  REQUIRE(fl.blocks().size() == 1 && fl.free_bytes() == m.size, where);
}

void random_case(size_t size, uint64_t seed, int steps) {
  const std::string where = "random size=" + std::to_string(size) + " seed=" + std::to_string(seed);
  std::mt19937_64 rng(seed);
  OiFreeList fl;
  Model m;
  fl.reset(size);
  m.reset(size);
  check_state(fl, m, where);
  const size_t menu[] = {0, 1, 255, 256, 257, 512, 4096, size, size / G * G, size / 2, size + 1};
  for (int s = 0; s < steps; ++s) {
    const unsigned op = rng() % 16;
    if (op < 8 || m.live.empty()) {
      size_t bytes;
      const unsigned pick = rng() % 16;
      if (pick < 11)
        bytes = menu[pick];
      else if (pick < 14)
        bytes = rng() % (size / 8 + 2);
      else
        bytes = rng() % (size + 1);
      do_alloc(fl, m, bytes, where);
    } else if (op < 14) {
      const size_t idx = rng() % m.live.size();
      const Live b = m.live[idx];
      do_release(fl, m, idx, where);
      const auto before = fl.blocks();
      fl.release(b.off, b.bytes);  // a second release of the same block
      REQUIRE(fl.blocks() == before, where);
    } else {
      bogus_releases(fl, m, rng, where);
    }
    if ((s & 255) == 255)  // drain now and then, so full and empty arenas both occur
      release_all_and_check(fl, m, rng, where);
  }
  release_all_and_check(fl, m, rng, where);
}

// The sequence of an n = 0 cell admitted between two others: the empty block
// shares its neighbour's offset, leaves first, and the neighbour's bytes must
// still come back.
void case_zero_byte_neighbour() {
  const std::string where = "zero_byte_neighbour";
  const size_t size = size_t(1) << 20;
  OiFreeList fl;
  fl.reset(size);
  REQUIRE(fl.alloc(4096) == 0, where);
  const size_t z = fl.alloc(0);
  REQUIRE(z != SIZE_MAX, where);
  REQUIRE(fl.alloc(65536) == 4096, where);
  fl.release(4096, 0);
  fl.release(z, 0);
  fl.release(4096, 65536);
  fl.release(0, 4096);
  REQUIRE(fl.blocks().size() == 1, where);
  REQUIRE(fl.blocks().begin()->first == 0 && fl.blocks().begin()->second == size, where);
  REQUIRE(fl.free_bytes() == size && fl.largest_free() == size, where);
  REQUIRE(fl.alloc(size) == 0, where);
}

// An empty cell waits for no memory: alloc(0) succeeds in a full arena and
// leaves no entry behind.
void case_zero_byte_in_full_arena() {
  const std::string where = "zero_byte_in_full_arena";
  const size_t size = 8192;
  OiFreeList fl;
  fl.reset(size);
  REQUIRE(fl.alloc(size) == 0, where);
  REQUIRE(fl.blocks().empty(), where);
  const size_t z = fl.alloc(0);
  REQUIRE(z != SIZE_MAX && z <= size, where);
  REQUIRE(fl.blocks().empty(), where);
  fl.release(z, 0);
  fl.release(0, 0);
  REQUIRE(fl.blocks().empty(), where);
  REQUIRE(fl.alloc(1) == SIZE_MAX, where);
  fl.release(0, size);
  REQUIRE(fl.blocks().size() == 1 && fl.free_bytes() == size, where);
}

// A block released between two free ones joins both; in front of and behind a
// live block it joins one.
void case_coalesce() {
  const std::string where = "coalesce";
  OiFreeList fl;
  fl.reset(4096);
  size_t o[4];
  for (size_t& x : o) x = fl.alloc(1000);  // 1024 each
  REQUIRE(o[0] == 0 && o[1] == 1024 && o[2] == 2048 && o[3] == 3072, where);
  fl.release(o[0], 1000);
  fl.release(o[2], 1000);
  REQUIRE(fl.blocks().size() == 2 && fl.largest_free() == 1024, where);
  fl.release(o[1], 1000);
  REQUIRE(fl.blocks().size() == 1 && fl.largest_free() == 3072, where);
  REQUIRE(fl.alloc(3072) == 0, where);
  fl.release(o[3], 1000);
  REQUIRE(fl.blocks().size() == 1 && fl.blocks().begin()->first == 3072, where);
  fl.release(0, 3072);
  REQUIRE(fl.blocks().size() == 1 && fl.free_bytes() == 4096, where);
}

}  // namespace

int main() {
  case_zero_byte_neighbour();
  case_zero_byte_in_full_arena();
  case_coalesce();
  int cases = 3;
  const size_t sizes[] = {256, 512, 4096, 65536, size_t(1) << 20, 1000, 65536 + 100};
  for (size_t size : sizes)
    for (uint64_t seed = 1; seed <= 6; ++seed, ++cases) random_case(size, seed, 1500);
  std::printf("OK %d cases, %d checks\n", cases, g_checks);
  return 0;
}
