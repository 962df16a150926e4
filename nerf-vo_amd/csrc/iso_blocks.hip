// Iso-surface of the block-sparse TSDF volume (include/nerfvo_hip.h section M; DESIGN.md "Block-sparse TSDF volume"): the
// edge-owned marching tetrahedra of iso.hip -- the per-point rules of iso_dev.h that iso.hip calls: ownership, case table,
// winding and position formula exist once, there -- on the lattice [8 tbx][8 tby][8 tbz] read through the block table.
// values = -tsdf, threshold 0, a sample is valid when its block is allocated and its weight reaches the threshold; a
// sample of an unallocated block is invalid.
//
// A workgroup owns one block of `order` (table indices, ascending) and walks its 512 points in local order, 256 at a
// time, so ranks inside a workgroup follow the rule's order.  It first stages the block with a halo of one sample on
// every side (10^3 values and validity bytes, read through the ids of the 27 blocks around it) into LDS; everything a
// point needs -- its cube's eight corners, the far ends of its seven edge kinds, the validity of its 27 neighbours --
// lies in that halo.  Per-point scratch (rank, edge mask, triangle count) and the per-block totals and bases are indexed
// by block ID, so a triangle finds a vertex owned by a point of a neighbouring block without a second table.
#include "nvo_kernels.h"
#include "../../include/nerfvo_hip.h"
#include "iso_dev.h"
#include "tsdf_dev.h"

namespace {

constexpr uint32_t kBlock = 256;
constexpr uint32_t kB = NVO_TSDF_BLOCK, kBlockVoxels = kB * kB * kB;
constexpr uint32_t kH = kB + 2, kHalo = kH * kH * kH;  // the block and one sample on every side
static_assert(kB == 8 && kBlockVoxels == 2 * kBlock, "two rounds of 256 points per block");

struct Halo {
    float val[kHalo];    // -tsdf; 0 where invalid
    uint8_t ok[kHalo];   // allocated and weight >= threshold
    int32_t nid[27];     // id of the block at offset (ox, oy, oz) in -1..1: [(ox+1)*9 + (oy+1)*3 + (oz+1)], -1: none
};

__device__ __forceinline__ uint32_t halo_index(uint32_t li, uint32_t lj, uint32_t lk) {  // of the block's own point
    return ((li + 1u) * kH + (lj + 1u)) * kH + (lk + 1u);
}

// stage the halo of block (bi, bj, bk); ends with a barrier
__device__ __forceinline__ void load_halo(const nvo_tsdf_blocks_iso_args& a, uint32_t bi, uint32_t bj, uint32_t bk, Halo& h) {
    if (threadIdx.x < 27u) {
        const int32_t x = (int32_t)bi + (int32_t)(threadIdx.x / 9u) - 1, y = (int32_t)bj + (int32_t)((threadIdx.x / 3u) % 3u) - 1,
                      z = (int32_t)bk + (int32_t)(threadIdx.x % 3u) - 1;
        int32_t id = -1;
        if (x >= 0 && y >= 0 && z >= 0 && x < (int32_t)a.tbx && y < (int32_t)a.tby && z < (int32_t)a.tbz) {
            id = a.table[((size_t)x * a.tby + (size_t)y) * a.tbz + (size_t)z];
            if (id < 0 || (uint32_t)id >= a.n_allocated) id = -1;
        }
        h.nid[threadIdx.x] = id;
    }
    __syncthreads();
    for (uint32_t c = threadIdx.x; c < kHalo; c += kBlock) {
        const uint32_t hx = c / (kH * kH), hy = (c / kH) % kH, hz = c % kH;
        // halo coordinate 0 is the last sample of the block before, 9 the first of the block after
        const uint32_t ox = hx == 0u ? 0u : (hx == kH - 1u ? 2u : 1u), oy = hy == 0u ? 0u : (hy == kH - 1u ? 2u : 1u),
                       oz = hz == 0u ? 0u : (hz == kH - 1u ? 2u : 1u);
        const int32_t id = h.nid[ox * 9u + oy * 3u + oz];
        float val = 0.f;
        uint8_t ok = 0;
        if (id >= 0) {
            const uint32_t local = ((((hx + 7u) & 7u) * kB) + ((hy + 7u) & 7u)) * kB + ((hz + 7u) & 7u);
            const size_t idx = (size_t)id * kBlockVoxels + local;
            ok = a.weight[idx] >= a.weight_threshold ? 1 : 0;  // a NaN fails
            val = ok ? -a.tsdf[idx] : 0.f;
        }
        h.val[c] = val;
        h.ok[c] = ok;
    }
    __syncthreads();
}

// the block of a workgroup: false when the entry of `order` is no allocated block of the table (workgroup-uniform)
__device__ __forceinline__ bool block_of(const nvo_tsdf_blocks_iso_args& a, uint32_t n_table, uint32_t& id, uint32_t& bi, uint32_t& bj,
                                         uint32_t& bk) {
    const int32_t tix = a.order[blockIdx.x];
    if (tix < 0 || (uint32_t)tix >= n_table) return false;
    const int32_t v = a.table[tix];
    if (v < 0 || (uint32_t)v >= a.n_allocated) return false;
    id = (uint32_t)v;
    bk = (uint32_t)tix % a.tbz;
    const uint32_t bij = (uint32_t)tix / a.tbz;
    bj = bij % a.tby;
    bi = bij / a.tby;
    return true;
}

// id of the block that holds the point at (li + dx, lj + dy, lk + dz), d in {0, 1}, and the point's local index there
__device__ __forceinline__ int32_t far_point(const Halo& h, uint32_t li, uint32_t lj, uint32_t lk, uint32_t dx, uint32_t dy, uint32_t dz,
                                             uint32_t& local) {
    const uint32_t x = li + dx, y = lj + dy, z = lk + dz;  // 0 .. 8
    local = (((x & 7u) * kB) + (y & 7u)) * kB + (z & 7u);
    return h.nid[(1u + (x >> 3)) * 9u + (1u + (y >> 3)) * 3u + (1u + (z >> 3))];
}

__global__ void __launch_bounds__(kBlock) k_tsdf_blocks_iso_count(const nvo_tsdf_blocks_iso_args a, uint32_t n_table) {
    __shared__ Halo h;
    __shared__ uint32_t lds[4];
    uint32_t id, bi, bj, bk;
    if (!block_of(a, n_table, id, bi, bj, bk)) return;
    load_halo(a, bi, bj, bk, h);
    uint32_t vrun = 0, trun = 0;
    for (uint32_t round = 0; round < 2; ++round) {
        const uint32_t local = round * kBlock + threadIdx.x;
        const uint32_t li = local >> 6, lj = (local >> 3) & 7u, lk = local & 7u;
        const uint32_t hc = halo_index(li, lj, lk);
        uint32_t in = 0;
#pragma unroll
        for (uint32_t m = 0; m < 8; ++m)
            in |= (h.val[hc + (kIsoCorner[m][0] * kH + kIsoCorner[m][1]) * kH + kIsoCorner[m][2]] > 0.f ? 1u : 0u) << m;
        const uint32_t differ = ((in & 1u) ? ~in : in) & 0xFEu;  // corners on the other side than the point
        uint32_t mask = 0, tris = 0;
        if (differ != 0u) {
            uint32_t nb = 0;  // bit (dx+1)*9 + (dy+1)*3 + (dz+1): the neighbour at that offset is valid
#pragma unroll
            for (uint32_t dx = 0; dx < 3; ++dx)
#pragma unroll
                for (uint32_t dy = 0; dy < 3; ++dy)
#pragma unroll
                    for (uint32_t dz = 0; dz < 3; ++dz)
                        nb |= (uint32_t)h.ok[hc + (dx * kH + dy) * kH + dz - (kH * kH + kH + 1u)] << (dx * 9u + dy * 3u + dz);
            iso_classify(in, differ, nb, mask, tris);
        }
        uint32_t vtot, ttot;
        const uint32_t vex = block_excl_scan(__popc(mask), lds, vtot);
        (void)block_excl_scan(tris, lds, ttot);
        const size_t p = (size_t)id * kBlockVoxels + local;
        a.vrank[p] = vrun + vex;
        a.mask[p] = (uint8_t)mask;
        a.tcount[p] = (uint8_t)tris;
        vrun += vtot;
        trun += ttot;
    }
    if (threadIdx.x == 0) {
        a.totals[id] = (int64_t)vrun;
        a.totals[(size_t)a.n_allocated + id] = (int64_t)trun;
    }
}

__global__ void __launch_bounds__(kBlock) k_tsdf_blocks_iso_emit(const nvo_tsdf_blocks_iso_args a, uint32_t n_table) {
    __shared__ Halo h;
    __shared__ uint32_t lds[4];
    uint32_t id, bi, bj, bk;
    if (!block_of(a, n_table, id, bi, bj, bk)) return;
    load_halo(a, bi, bj, bk, h);
    const uint64_t vbase = (uint64_t)a.vertex_base[id], fbase = (uint64_t)a.face_base[id];
    const float step[3] = {a.voxel_size, a.voxel_size, a.voxel_size};
    uint32_t trun = 0;
    for (uint32_t round = 0; round < 2; ++round) {
        const uint32_t local = round * kBlock + threadIdx.x;
        const uint32_t li = local >> 6, lj = (local >> 3) & 7u, lk = local & 7u;
        const uint32_t hc = halo_index(li, lj, lk);
        const size_t p = (size_t)id * kBlockVoxels + local;
        const uint32_t mask = a.mask[p], tris = a.tcount[p];
        if (mask != 0u) {
            uint64_t vid = vbase + a.vrank[p];
            const float va = h.val[hc];
            const size_t ca = (size_t)id * (3 * kBlockVoxels) + local;
            const uint32_t i = bi * kB + li, j = bj * kB + lj, k = bk * kB + lk;  // the GLOBAL lattice index
            for (uint32_t kind = 0; kind < 7; ++kind) {
                if (!((mask >> kind) & 1u)) continue;
                const uint32_t dx = kIsoKind[kind][0], dy = kIsoKind[kind][1], dz = kIsoKind[kind][2];
                const float vb = h.val[hc + (dx * kH + dy) * kH + dz];
                const float t = iso_cut(va, vb, 0.f);
                const float3 pos = iso_vertex(i, j, k, dx, dy, dz, t, a.lower, step);
                uint32_t lb;
                const int32_t idb = far_point(h, li, lj, lk, dx, dy, dz, lb);  // allocated: the edge lies in an active cube
                if (vid < a.n_vertices && idb >= 0) {  // (always, when vertex_base is the prefix sum of this count's totals)
                    float* o = a.vertices + (size_t)vid * 3;
                    o[0] = pos.x;
                    o[1] = pos.y;
                    o[2] = pos.z;
                    const size_t cb = (size_t)idb * (3 * kBlockVoxels) + lb;
                    uint8_t* oc = a.colors + (size_t)vid * 3;
#pragma unroll
                    for (uint32_t ch = 0; ch < 3; ++ch) {
                        const float c = (1.f - t) * a.color[ca + ch * kBlockVoxels] + t * a.color[cb + ch * kBlockVoxels];
                        oc[ch] = (uint8_t)fminf(fmaxf(rintf(c), 0.f), 255.f);  // a NaN becomes 0
                    }
                }
                ++vid;
            }
        }
        uint32_t ttot;
        const uint32_t tex = block_excl_scan(tris, lds, ttot);
        if (tris != 0u) {  // the cube at the point is active: all eight corners are valid, their blocks allocated
            uint32_t in = 0;
#pragma unroll
            for (uint32_t m = 0; m < 8; ++m)
                in |= (h.val[hc + (kIsoCorner[m][0] * kH + kIsoCorner[m][1]) * kH + kIsoCorner[m][2]] > 0.f ? 1u : 0u) << m;
            iso_emit_faces(in, fbase + trun + tex, a.n_faces, a.faces, [&] __device__(uint32_t oc, uint32_t kind) {
                uint32_t lq;
                const int32_t idq = far_point(h, li, lj, lk, kIsoCorner[oc][0], kIsoCorner[oc][1], kIsoCorner[oc][2], lq);
                if (idq < 0) return (int32_t)-1;  // a block that is not allocated
                const size_t q = (size_t)idq * kBlockVoxels + lq;
                const uint32_t below = (uint32_t)a.mask[q] & ((1u << kind) - 1u);
                return (int32_t)((uint64_t)a.vertex_base[idq] + a.vrank[q] + __popc(below));
            });
        }
        trun += ttot;
    }
}

int iso_blocks_check(const nvo_tsdf_blocks_iso_args& a, const char* what, uint64_t* n_table) {
    if (int rc = tsdf_table_check(what, a.tbx, a.tby, a.tbz, n_table)) return rc;
    NVO_REQUIRE(a.n_allocated <= NVO_TSDF_BLOCKS_MAX_ALLOCATED && a.n_blocks <= a.n_allocated,
                "%s: %u blocks to walk of %u allocated, of at most %u", what, a.n_blocks, a.n_allocated, NVO_TSDF_BLOCKS_MAX_ALLOCATED);
    NVO_REQUIRE(a.voxel_size > 0.f && a.voxel_size < INFINITY, "%s: voxel_size %g must be positive and finite", what,
                (double)a.voxel_size);
    if (a.n_blocks == 0) return NVO_OK;
    NVO_REQUIRE(a.table && a.tsdf && a.weight && a.order && a.totals && a.vrank && a.mask && a.tcount, "%s: NULL argument", what);
    return NVO_OK;
}

}  // namespace

extern "C" {

int nvo_tsdf_blocks_iso_count(nvo_stream_t stream, const nvo_tsdf_blocks_iso_args* args) {
    NVO_REQUIRE(args != nullptr, "tsdf_blocks_iso_count: args is NULL");
    const nvo_tsdf_blocks_iso_args a = *args;
    uint64_t n_table;
    if (int rc = iso_blocks_check(a, "tsdf_blocks_iso_count", &n_table)) return rc;
    if (a.n_blocks == 0) return NVO_OK;
    NVO_PROF(stream, "tsdf_blocks_iso_count");
    NVO_LAUNCH(k_tsdf_blocks_iso_count, dim3(a.n_blocks), dim3(kBlock), 0, (hipStream_t)stream, a, (uint32_t)n_table);
    NVO_CHECK_LAUNCH();
    return NVO_OK;
}

int nvo_tsdf_blocks_iso_emit(nvo_stream_t stream, const nvo_tsdf_blocks_iso_args* args) {
    NVO_REQUIRE(args != nullptr, "tsdf_blocks_iso_emit: args is NULL");
    const nvo_tsdf_blocks_iso_args a = *args;
    uint64_t n_table;
    if (int rc = iso_blocks_check(a, "tsdf_blocks_iso_emit", &n_table)) return rc;
    if (int rc = iso_counts_check("tsdf_blocks_iso_emit", a.n_vertices, a.n_faces)) return rc;
    if (a.n_blocks == 0 || (a.n_vertices == 0 && a.n_faces == 0)) return NVO_OK;
    NVO_REQUIRE(a.color && a.vertex_base && a.face_base && (a.n_vertices == 0 || (a.vertices && a.colors)) && (a.faces || a.n_faces == 0),
                "tsdf_blocks_iso_emit: NULL color, vertex_base, face_base, vertices, colors or faces");
    NVO_PROF(stream, "tsdf_blocks_iso_emit");
    NVO_LAUNCH(k_tsdf_blocks_iso_emit, dim3(a.n_blocks), dim3(kBlock), 0, (hipStream_t)stream, a, (uint32_t)n_table);
    NVO_CHECK_LAUNCH();
    return NVO_OK;
}

}  // extern "C"
