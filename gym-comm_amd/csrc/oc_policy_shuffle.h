// oc_policy_shuffle.h -- the epoch permutation of the PPO train sequence, stated once (the contract in
// prose: include/oc_policy.h, "the permutation").  Read by the shuffle kernel (oc_policy_train.hip), by
// oc_policy_ppo_perm_host and, alone, by a host compiler (tests/policy_shuffle_driver.cc): plain C++,
// no HIP header.
//
// perm(seed, epoch, N, i) is a bijection of 0 .. N - 1 by construction: a balanced Feistel network
// is a bijection of 0 .. 2^bits - 1 whatever its round function is, and following it from a point
// below N until it comes back below N (cycle walking) restricts a bijection of a set to a bijection
// of a subset.  Every element is computed on its own, from (seed, epoch, N) alone.
#ifndef OC_POLICY_SHUFFLE_H
#define OC_POLICY_SHUFFLE_H
#include <stdint.h>

#ifdef __HIP__
#define OC_SHUF_HD __attribute__((host)) __attribute__((device))
#else
#define OC_SHUF_HD
#endif

namespace ocpol {

constexpr int SHUFFLE_ROUNDS = 4;
constexpr int32_t SHUFFLE_MAX_N = 1 << 30;   // bits <= 30: every word below fits 32 bits
// The walk from a point below N meets at most 2^bits - N < 3 N points outside before it is back
// inside, so it ends for every bijection; each step lands inside with a chance above 1/4, and the
// tests print the longest walk they see (tens of steps).  The cap is there so that a BUG in the map
// -- a network that is no bijection -- ends in an error word instead of a loop without end.
constexpr int SHUFFLE_WALK_CAP = 4096;

// murmur3's 32-bit finaliser
OC_SHUF_HD constexpr uint32_t fmix32(uint32_t h) {
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}

// the smallest even number of bits, at least 2, whose range holds 0 .. N - 1: the domain is below 4 N
OC_SHUF_HD constexpr int shuffle_bits(int32_t N) {
  int b = 2;
  while (((int64_t)1 << b) < (int64_t)N) b += 2;
  return b;
}

OC_SHUF_HD constexpr uint32_t shuffle_key(uint32_t seed, uint32_t epoch, int r) {
  return fmix32(seed ^ (0x9E3779B9u * (4u * epoch + (uint32_t)r + 1u)));
}

struct Shuffle {
  int32_t N;
  int half;                       // bits of one half of the word
  uint32_t mask;                  // 2^half - 1
  uint32_t key[SHUFFLE_ROUNDS];
  OC_SHUF_HD constexpr Shuffle(uint32_t seed, uint32_t epoch, int32_t N_)
      : N(N_), half(shuffle_bits(N_) / 2), mask((1u << (shuffle_bits(N_) / 2)) - 1u), key{} {
    for (int r = 0; r < SHUFFLE_ROUNDS; r++) key[r] = shuffle_key(seed, epoch, r);
  }
  // one pass of the network over the whole domain 0 .. 2^(2 half) - 1
  OC_SHUF_HD constexpr uint32_t pass(uint32_t x) const {
    uint32_t L = x >> half, R = x & mask;
    for (int r = 0; r < SHUFFLE_ROUNDS; r++) {
      const uint32_t t = L ^ (fmix32(R ^ key[r]) & mask);
      L = R, R = t;
    }
    return (L << half) | R;
  }
  // perm[i] for 0 <= i < N, or -1 when the walk reaches the cap; *steps (optional): passes taken
  OC_SHUF_HD constexpr int32_t at(int32_t i, int *steps = nullptr) const {
    uint32_t x = (uint32_t)i;
    for (int k = 1; k <= SHUFFLE_WALK_CAP; k++) {
      x = pass(x);
      if (x < (uint32_t)N) {
        if (steps != nullptr) *steps = k;
        return (int32_t)x;
      }
    }
    if (steps != nullptr) *steps = SHUFFLE_WALK_CAP;
    return -1;
  }
};

}  // namespace ocpol
#endif
