// group_sort.hpp -- a bitonic sort of 64-bit words in LDS by a group of G lanes: one wave64 (ordered by wave-scope fences only, no
// workgroup barrier) or one kBlock workgroup.  Shared by walk_visit.hip (PinSAGE visit counts) and pool.hip (per-graph top-k).
#pragma once
#include "common.hpp"

namespace pglamd {

// All lanes of the group have finished their LDS accesses before any goes on.  A wave's DS instructions execute in order,
// so inside one wave only the compiler has to be kept from moving accesses across this point.
template <int G>
__device__ __forceinline__ void group_sync() {
    if (G == kWave) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    } else {
        __syncthreads();
    }
}

// Bitonic sort of a[0 .. n2) (n2 a power of two) by the G lanes of the group; lane = the lane's number inside the group.
template <int G, bool DESCENDING>
__device__ __forceinline__ void group_sort(uint64_t* a, int n2, int lane) {
    for (int k = 2; k <= n2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int p = lane; p < (n2 >> 1); p += G) {
                const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), l = i | j;      // l < n2: i < n2 has bit j clear
                const uint64_t x = a[i], y = a[l];
                const bool up = ((i & k) == 0) != DESCENDING;
                if ((x > y) == up) { a[i] = y; a[l] = x; }
            }
            group_sync<G>();
        }
    }
}

}  // namespace pglamd
