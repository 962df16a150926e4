// The per-point rules of the edge-owned extractor, shared by its two forms: iso.hip (a dense lattice) and iso_blocks.hip
// (the block-sparse TSDF volume).  Each rule exists here and nowhere else; the two forms differ in where a point's samples,
// validity and scratch live.  Both launch 256-thread workgroups.
#pragma once
#include "nvo_common.h"
#include "iso_tables.h"

#include <math.h>

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

// case of tetrahedron t from the cube's inside bits: bit m is tetrahedron corner m
static __device__ __forceinline__ uint32_t iso_tet_case(uint32_t in, uint32_t t) {
    uint32_t row, c = 0;
    __builtin_memcpy(&row, kIsoTet[t], 4);  // the four corners in ONE (scalar) load; byte m is corner m (EXPERIMENTS.md 23)
#pragma unroll
    for (uint32_t m = 0; m < 4; ++m) c |= ((in >> ((row >> (8 * m)) & 0xFFu)) & 1u) << m;
    return c;
}

// A point's 7-bit mask of the cut edges it owns and the triangle count of its cube, from the cube's inside bits `in`,
// the corners `differ` that exist and lie on the other side than the point (corner 0), and the neighbourhood `nb`
// (bit (dx+1)*9 + (dy+1)*3 + (dz+1): the neighbour at that offset is in the lattice and valid).
static __device__ __forceinline__ void iso_classify(uint32_t in, uint32_t differ, uint32_t nb, uint32_t& mask, uint32_t& tris) {
#pragma unroll
    for (uint32_t kind = 0; kind < 7; ++kind) {
        if (!((differ >> kIsoKindCorner[kind]) & 1u)) continue;
        const uint32_t dx = kIsoKind[kind][0], dy = kIsoKind[kind][1], dz = kIsoKind[kind][2];
        // cubes with both ends among their corners: minimum corner = point - o, o = 0 on the edge's axes
        bool any = false;
        for (uint32_t ox = 0; ox <= 1u - dx; ++ox)
            for (uint32_t oy = 0; oy <= 1u - dy; ++oy)
                for (uint32_t oz = 0; oz <= 1u - dz; ++oz) any = any || cube_active(nb, ox, oy, oz);
        mask |= (any ? 1u : 0u) << kind;
    }
    if (cube_active(nb, 0, 0, 0)) {
#pragma unroll
        for (uint32_t t = 0; t < 6; ++t) tris += kIsoTriCount[t][iso_tet_case(in, t)];
    }
}

// where the edge from a sample va to a sample vb crosses the threshold, as a share of the edge
static __device__ __forceinline__ float iso_cut(float va, float vb, float threshold) {
    const float t = (threshold - va) / (vb - va);
    return fminf(fmaxf(t, 0.f), 1.f);
}

// position of the vertex at share t of the edge from lattice point (i, j, k) towards (i + dx, j + dy, k + dz)
static __device__ __forceinline__ float3 iso_vertex(uint32_t i, uint32_t j, uint32_t k, uint32_t dx, uint32_t dy, uint32_t dz, float t,
                                                    const float* lower, const float* step) {
    const float gx = (float)i + (dx ? t : 0.f), gy = (float)j + (dy ? t : 0.f), gz = (float)k + (dz ? t : 0.f);
    return make_float3(lower[0] + gx * step[0], lower[1] + gy * step[1], lower[2] + gz * step[2]);
}

// The triangles of a cube with inside bits `in`, tetrahedra 0..5, from face f on.  lookup(owner corner, kind) is the id of
// the vertex on the edge of that kind owned by the point at that corner of the cube, or -1: the face is then skipped,
// and so is every face from n_faces on; f advances either way.  Pass a `[&] __device__` lambda: a plain one is a
// host-device function, and a table of iso_tables.h that such a function names stays visible to the host, which keeps
// the compiler from folding its entries at constant indices in every kernel of the file.
template <class Lookup>
static __device__ __forceinline__ void iso_emit_faces(uint32_t in, uint64_t f, uint64_t n_faces, int32_t* faces, Lookup lookup) {
    for (uint32_t t = 0; t < 6; ++t) {
        const uint32_t c = iso_tet_case(in, t);
        const uint32_t nt = kIsoTriCount[t][c];
        for (uint32_t r = 0; r < nt; ++r) {
            int32_t ids[3];
#pragma unroll
            for (uint32_t v = 0; v < 3; ++v) {
                const uint32_t e = kIsoTriEdge[t][c][3 * r + v];
                ids[v] = lookup((e >> 3) & 7u, e & 7u);
            }
            if (f < n_faces && ids[0] >= 0 && ids[1] >= 0 && ids[2] >= 0) {
                int32_t* o = faces + (size_t)f * 3;
                o[0] = ids[0];
                o[1] = ids[1];
                o[2] = ids[2];
            }
            ++f;
        }
    }
}

// host: int32 face indices and the prefix sums' range
static inline int iso_counts_check(const char* what, uint64_t n_vertices, uint64_t n_faces) {
    NVO_REQUIRE(n_vertices < (1ull << 31) && n_faces < (1ull << 31),
                "%s: %llu vertices and %llu faces: each must stay below 2^31 (int32 face indices)", what,
                (unsigned long long)n_vertices, (unsigned long long)n_faces);
    return NVO_OK;
}
