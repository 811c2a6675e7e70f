// tests/cpp/facade_nearest.cpp — helper of tests/test_nearest_cpu.py and tests/test_gpu_nearest.py: IntervalTree::find_nearest
// (include/binary/algorithm/interval_tree.hpp) against a host brute force, for uint32_t and int64_t keys, with queries
// inside, across and wholly outside the tree's coordinate window, with and without max_distance.
//   usage: facade_nearest          prints "facade_nearest: <n> checks, <k> failed"; exit status 0 iff k == 0
#include <binary/algorithm/all.hpp>
#include <cstdint>
#include <cstdio>
#include <optional>
#include <vector>

using namespace binary::algorithm::tree;

namespace {

int g_checks = 0, g_failed = 0;

std::uint64_t g_state = 7;
std::uint64_t rnd(std::uint64_t n) {  // splitmix64, uniform in [0, n)
  std::uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return n ? z % n : 0;
}

// distance in key units, as an unsigned 64-bit number (the keys here stay far from the limits of their types)
template <typename K> std::uint64_t dist(K ql, K qh, K l, K h) {
  const long double a = static_cast<long double>(ql) - static_cast<long double>(h);
  const long double b = static_cast<long double>(l) - static_cast<long double>(qh);
  const long double d = a > b ? a : b;
  return d > 0 ? static_cast<std::uint64_t>(d) : 0u;
}

// index of the nearest interval (smallest distance, then smallest index) within max_d, or -1
template <typename K>
long brute(const std::vector<BaseInterval<K>> &iv, K ql, K qh, std::optional<std::uint64_t> max_d) {
  long best = -1;
  std::uint64_t bd = 0;
  for (std::size_t i = 0; i < iv.size(); ++i) {
    const std::uint64_t d = dist(ql, qh, iv[i].low, iv[i].high);
    if (max_d && d > *max_d) continue;
    if (best < 0 || d < bd) {
      best = static_cast<long>(i);
      bd = d;
    }
  }
  return best;
}

// intervals in [origin, origin + span + maxlen); queries far below reach down to origin - room - 2 maxlen
template <typename K> void run(K origin, K span, K room, std::size_t n, std::size_t nq, K maxlen, const char *what) {
  using Node = IntervalNode<BaseInterval<K>>;
  IntervalTree<Node> tree{};
  std::vector<BaseInterval<K>> iv;
  for (std::size_t i = 0; i < n; ++i) {
    const K lo = origin + static_cast<K>(rnd(static_cast<std::uint64_t>(span)));
    const K hi = lo + static_cast<K>(rnd(static_cast<std::uint64_t>(maxlen)));
    iv.emplace_back(lo, hi);
    if (i % 17 == 3) iv.push_back(iv.back());  // duplicates: ties go to the one inserted first
  }
  for (auto const &i : iv) tree.insert_node(i.low, i.high);
  // empty-handed only when there is nothing to find
  IntervalTree<Node> empty{};
  ++g_checks;
  if (empty.find_nearest(BaseInterval<K>{origin, origin})) {
    ++g_failed;
    std::printf("%s: an empty tree found something\n", what);
  }
  for (std::size_t k = 0; k < nq; ++k) {
    // a third inside, a third across the window's edges, a third wholly outside (far below or far above)
    K ql;
    const std::uint64_t kind = k % 3;
    if (kind == 0) ql = origin + static_cast<K>(rnd(static_cast<std::uint64_t>(span)));
    else if (kind == 1) ql = origin - static_cast<K>(rnd(static_cast<std::uint64_t>(span) / 4)) + (k % 2 ? span : K{0});
    else ql = k % 2 ? origin - static_cast<K>(1 + rnd(static_cast<std::uint64_t>(room))) - maxlen * 2
                     : origin + span * 5 + static_cast<K>(rnd(static_cast<std::uint64_t>(span)));
    const K qh = ql + static_cast<K>(rnd(static_cast<std::uint64_t>(maxlen) * 2));
    const BaseInterval<K> q{ql, qh};
    for (int m = 0; m < 3; ++m) {
      std::optional<std::uint64_t> md;
      if (m == 1) md = 0;
      if (m == 2) md = rnd(static_cast<std::uint64_t>(maxlen) * 4);
      const long exp = brute(iv, ql, qh, md);
      const auto got = md ? tree.find_nearest(q, static_cast<K>(*md)) : tree.find_nearest(q);
      ++g_checks;
      bool ok = got.has_value() == (exp >= 0);
      if (ok && got) {
        const auto &e = iv[static_cast<std::size_t>(exp)];
        ok = got->low == e.low && got->high == e.high;
      }
      if (!ok) {
        ++g_failed;
        if (g_failed < 20)
          std::printf("%s: query %lld-%lld max %lld: got %s, expected %s\n", what, static_cast<long long>(ql),
                      static_cast<long long>(qh), md ? static_cast<long long>(*md) : -1ll, got ? "an interval" : "none",
                      exp >= 0 ? "an interval" : "none");
      }
    }
  }
}

}  // namespace

int main() {
  run<std::uint32_t>(1'000'000u, 400'000u, 900'000u, 3000, 600, 2'000u, "uint32");
  run<std::uint32_t>(10'000u, 60u, 5'000u, 40, 200, 5u, "uint32 small");
  run<std::int64_t>(1'000'000'000'000ll, 3'000'000ll, 999'000'000'000ll, 3000, 600, 5'000ll, "int64");
  run<std::int64_t>(-2'000'000'000'000ll, 50'000ll, 7'000'000'000'000ll, 200, 300, 100ll, "int64 negative");
  std::printf("facade_nearest: %d checks, %d failed\n", g_checks, g_failed);
  return g_failed == 0 ? 0 : 1;
}
