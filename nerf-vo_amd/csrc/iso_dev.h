// Device helpers shared by the two forms of the edge-owned extractor: iso.hip (a dense lattice) and iso_blocks.hip (the
// block-sparse TSDF volume).  Both launch 256-thread workgroups.
#pragma once
#include "nvo_common.h"

// exclusive prefix sum of v over the 256 threads and the total; lds holds 4 words and is free again on return
static __device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t* lds, uint32_t& total) {
    const uint32_t incl = nvo_wave_incl_scan(v);
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 63u) lds[wave] = incl;
    __syncthreads();
    const uint32_t w0 = lds[0], w1 = lds[1], w2 = lds[2], w3 = lds[3];
    __syncthreads();
    total = w0 + w1 + w2 + w3;
    const uint32_t before = (wave > 0 ? w0 : 0u) + (wave > 1 ? w1 : 0u) + (wave > 2 ? w2 : 0u);
    return before + incl - v;
}

// the cube whose minimum corner is the point minus (ox, oy, oz) is active
static __device__ __forceinline__ bool cube_active(uint32_t nb, uint32_t ox, uint32_t oy, uint32_t oz) {
    constexpr uint32_t kCube = 1u | 2u | 8u | 16u | 512u | 1024u | 4096u | 8192u;  // offsets {0,1}^3 from the minimum corner
    const uint32_t start = (1u - ox) * 9u + (1u - oy) * 3u + (1u - oz);
    return ((nb >> start) & kCube) == kCube;
}
