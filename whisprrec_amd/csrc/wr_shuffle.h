// wr_shuffle.h — the keyed bijection of [0, n) shared by the epoch shuffle (wr_sampler.hip) and the SGL view builder
// (wr_views.hip): an alternating Feistel network on ceil(log2 n) bits (the two halves take turns being XORed with a splitmix64
// hash of the other half, the round number and the key; kShuffleRounds rounds) with cycle walking (re-apply until the value is
// < n; the domain is < 2n for n >= 4, so < 2 evaluations on average).  Evaluated per element: no sort, no order array.
// oracle.epoch_permutation_at restates it bit for bit; that is the project's own generator restated, so what holds the ORDER to
// a uniform one is the battery of tests/test_epoch_prep_contract.py (bucket tables, successors, fixed points, consecutive epochs,
// batch composition; 2, 3 and 4 rounds fail it, 6 could not be told from 8).  Known limit: the halves are 1 to 2 bits wide below
// n = 16 and the single-position marginals are then measurably not uniform (z = 7.2 / 4.6 / 2.6 at n = 5 / 6 / 9 over 20,000
// epochs, cell probabilities off by up to 6 %); from n = 16 up they pass (asserted at n = 16, 17, 32, 33, 64).  An epoch of
// fewer than 16 rows does not occur in the data this project targets.
#pragma once
#include "wr_common.h"

namespace wr {

constexpr int kShuffleRounds = 8;

__host__ __device__ __forceinline__ uint64_t shuffle_index(uint64_t i, uint64_t n, unsigned bits, uint64_t key) {
    const unsigned a = bits >> 1, b = bits - a;              // widths of the high and the low half (b >= a >= 1)
    const uint64_t mask_a = (uint64_t(1) << a) - 1, mask_b = (uint64_t(1) << b) - 1;
    uint64_t x = i;
    do {
        uint64_t hi = x >> b, lo = x & mask_b;
#pragma unroll
        for (int r = 0; r < kShuffleRounds; ++r) {
            if ((r & 1) == 0) hi ^= mix64(key ^ (lo * 0xD1B54A32D192ED03ull + (uint64_t)r)) & mask_a;
            else lo ^= mix64(key ^ (hi * 0xD1B54A32D192ED03ull + (uint64_t)r)) & mask_b;
        }
        x = (hi << b) | lo;
    } while (x >= n);
    return x;
}

static inline unsigned shuffle_bits(int64_t n) {
    unsigned bits = 2;
    while (bits < 62 && (int64_t(1) << bits) < n) ++bits;
    return bits;
}

// the network's key of (seed, epoch); `epoch` is any 64-bit stream number
static inline uint64_t shuffle_key(uint64_t seed, uint64_t epoch) {
    return mix64(mix64(seed ^ (epoch * 0x9E3779B97F4A7C15ull)) ^ 0x5DEECE66Dull);
}

}  // namespace wr
