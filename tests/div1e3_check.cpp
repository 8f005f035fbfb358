// Exhaustive host check of victoriametrics_amd/csrc/vm_div1e3.h: the
// division-free sequence against a true IEEE division for every integer x in
// [0, 2^32) and for every negated x in (-2^32, 0).  Built and run by test_div1e3_host.py.
//
// usage: div1e3_check [threads]      prints "mismatches <count>"
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "vm_div1e3.h"

static inline uint64_t bits(double d) {
  uint64_t u;
  std::memcpy(&u, &d, sizeof u);
  return u;
}

static uint64_t check_range(uint64_t lo, uint64_t hi) {
  uint64_t bad = 0;
  for (uint64_t x = lo; x < hi; x++) {
    double xd = (double)(int64_t)x;
    bad += bits(vm_div1e3_small(xd)) != bits(xd / 1e3);
    // -0.0 is no integer's conversion: the negated range starts at -1
    if (x) bad += bits(vm_div1e3_small(-xd)) != bits(-xd / 1e3);
  }
  return bad;
}

int main(int argc, char** argv) {
  int nthreads = argc > 1 ? std::atoi(argv[1]) : 8;
  if (nthreads < 1) nthreads = 1;
  const uint64_t total = 1ull << 32;
  // sanity: the check must be able to see a mismatch at all (the bare
  // multiply is known to be off for many x)
  uint64_t naive_bad = 0;
  for (uint64_t x = 0; x < 100000; x++)
    naive_bad += bits((double)x * 0.001) != bits((double)x / 1e3);
  if (naive_bad == 0) {
    std::printf("self-check failed: bare multiply never mismatched\n");
    return 2;
  }
  std::atomic<uint64_t> bad{0};
  std::vector<std::thread> pool;
  for (int t = 0; t < nthreads; t++) {
    uint64_t lo = total / nthreads * t;
    uint64_t hi = (t == nthreads - 1) ? total : total / nthreads * (t + 1);
    pool.emplace_back([lo, hi, &bad] { bad += check_range(lo, hi); });
  }
  for (auto& th : pool) th.join();
  std::printf("mismatches %llu\n", (unsigned long long)bad.load());
  return bad.load() == 0 ? 0 : 1;
}
