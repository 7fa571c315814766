// sample_core.hpp -- the neighbour sampler's draw shared by the kernels (sampling.hip, sampling_rel.hip) and the host twin
// (host_ops.cpp: pglamd_sample_relations_host), so the three cannot drift: the same counter-based hash, the same Floyd step, the
// same per-relation seed.
//
// A node v of degree deg > k >= 0 picks k of its row's POSITIONS 0 .. deg - 1 without replacement by Floyd's algorithm: draw
// c = 0 .. k - 1 has j = deg - k + c, r = mix64(seed ^ mix64(v * 0x100000001B3 + c)), t = r % (j + 1); a t an earlier draw of this
// node produced becomes j.  Every draw is a pure function of (seed, node id, draw number): results depend neither on the grid nor
// on the seed's position in the batch.  tests/sampling_defs.py restates it in numpy, bit for bit.
#pragma once
#include <stdint.h>

#if defined(__HIP__)
#define PGLAMD_SAMPLE_HD __host__ __device__ inline
#else
#define PGLAMD_SAMPLE_HD inline
#endif

namespace pglamd {
namespace sample {

constexpr int kMaxSample = 64;         // Floyd's set lives in registers / a per-lane array
constexpr int kMaxRelations = 64;      // PGLAMD_SAMPLE_MAX_RELATIONS: the fan-outs travel in the kernel's argument block

PGLAMD_SAMPLE_HD uint64_t mix64(uint64_t z) {        // splitmix64 finaliser
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// The seed relation r of a relation-stacked index samples with.  Mixed per relation because a draw is a function of (seed, node,
// draw number) alone: under one shared seed a node whose rows have equal lengths under two relations would pick the same positions
// in both.
PGLAMD_SAMPLE_HD uint64_t relation_seed(uint64_t seed, int64_t r) { return mix64(seed ^ mix64((uint64_t)r)); }

// Draw number c (0 <= c < k) of node v: the position it adds to chosen[0 .. c), the positions of the earlier draws.
PGLAMD_SAMPLE_HD int64_t floyd_draw(uint64_t seed, int64_t v, int64_t deg, int64_t k, int c, const int64_t* chosen) {
    const int64_t j = deg - k + c;
    const uint64_t r = mix64(seed ^ mix64((uint64_t)v * 0x100000001B3ull + (uint64_t)c));
    const int64_t t = (int64_t)(r % (uint64_t)(j + 1));
    bool dup = false;
    for (int q = 0; q < c; ++q) dup |= (chosen[q] == t);
    return dup ? j : t;
}

// How many entries node v contributes under fan-out k: the whole row when k < 0 or deg <= k, else k.
PGLAMD_SAMPLE_HD int64_t sample_count(int64_t deg, int64_t k) { return (k < 0 || deg <= k) ? deg : k; }

}  // namespace sample
}  // namespace pglamd
