// policy_shuffle_driver.cc -- gym-comm_amd/csrc/oc_policy_shuffle.h alone, by a host compiler under the
// address and undefined-behaviour sanitizers (tests/test_ppo_train_cpu.py): the epoch permutation is
// checked to be a bijection of 0 .. N - 1, exhaustively for every N <= 2048 and for the sizes the
// Python tests use, over several seeds and epochs; no walk may reach the cap.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../gym-comm_amd/csrc/oc_policy_shuffle.h"

using namespace ocpol;

static int failures = 0;
static int longest = 0;

static void check(uint32_t seed, uint32_t epoch, int32_t N) {
  const Shuffle sh(seed, epoch, N);
  std::vector<unsigned char> seen((size_t)N, 0);
  for (int32_t i = 0; i < N; i++) {
    int steps = 0;
    const int32_t p = sh.at(i, &steps);
    if (steps > longest) longest = steps;
    if (p < 0 || p >= N || seen[(size_t)(p < 0 || p >= N ? 0 : p)]) {
      if (failures++ < 20) printf("FAILED seed %u epoch %u N %d: element %d -> %d\n", seed, epoch, N, i, p);
      continue;
    }
    seen[(size_t)p] = 1;
  }
}

int main() {
  static_assert(shuffle_bits(1) == 2 && shuffle_bits(4) == 2 && shuffle_bits(5) == 4 && shuffle_bits(16) == 4 &&
                    shuffle_bits(17) == 6 && shuffle_bits(SHUFFLE_MAX_N) == 30,
                "the domain: the smallest even number of bits, at least 2, that holds N");
  static_assert(fmix32(0u) == 0u && fmix32(1u) == 0x514E28B7u, "murmur3's finaliser");
  const uint32_t seeds[] = {0u, 1u, 0x5EEDu, 0xFFFFFFFFu};
  for (int32_t N = 1; N <= 2048; N++)
    for (uint32_t seed : seeds)
      for (uint32_t epoch = 0; epoch < 2; epoch++) check(seed, epoch, N);
  const int32_t sizes[] = {1, 2, 3, 5, 64, 210, 4097, 65537, (1 << 20) + 1};
  for (int32_t N : sizes)
    for (uint32_t seed : seeds)
      for (uint32_t epoch = 0; epoch < 4; epoch++) check(seed, epoch, N);
  check(7u, 0xFFFFFFFFu, 1000);   // the key schedule wraps
  printf("longest walk: %d passes (cap %d)\n", longest, SHUFFLE_WALK_CAP);
  if (longest >= SHUFFLE_WALK_CAP) failures++;
  printf("failures: %d\n", failures);
  return failures != 0;
}
