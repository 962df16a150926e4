// TSDF fusion into a block-sparse volume (DESIGN.md "Block-sparse TSDF volume"; include/nerfvo_hip.h section M): the
// lattice of tsdf.hip cut into blocks of 8 x 8 x 8 voxels behind a dense block table, the shape of the reference's Open3D
// VoxelBlockGrid.  Two kernels:
//
//   k_tsdf_blocks_touch      which blocks does each frame's truncation band touch?  One thread per pixel walks the band
//                            of its depth in steps of half a voxel and marks the blocks within rho (L-infinity) of every
//                            sample with the frame's bit -- an integer atomic OR, so the marks do not depend on any order.
//                            tests/helpers/tsdf_blocks_oracle.py restates the arithmetic in float32 numpy, operation for
//                            operation (the library is built with -ffp-contract=off; sqrtf and the divisions are correctly
//                            rounded), and the sets are equal bit for bit.
//   k_tsdf_blocks_integrate  a workgroup owns one listed block (512 voxels, two per thread, z fastest) and applies the
//                            frames of the block's mask in table order by the per-voxel rule of tsdf_dev.h
//                            (tsdf_fuse_voxel: the function k_tsdf_integrate calls, here with the block's channel
//                            stride), so the result is bitwise independent of how frames are cut into launches.
//
// Bounds: the launchers check the table's size, K, the frame size and the pointers; the kernels predicate every table
// index, list entry and block id (an entry that fails is skipped), and a block index is compared as a float against the
// table's extent BEFORE it is converted to an integer (a NaN or infinite world coordinate marks nothing).
#include "nvo_kernels.h"
#include "tsdf_dev.h"

namespace {

constexpr int kBlock = 256;
constexpr uint32_t kMaxGrid = 2048;
constexpr uint32_t kMaxFrames = NVO_TSDF_MAX_FRAMES;
constexpr uint32_t kB = NVO_TSDF_BLOCK, kBlockVoxels = kB * kB * kB;
constexpr uint32_t kMaxSamples = 4096;
static_assert(kB == 8 && kBlockVoxels == 2 * kBlock, "two voxels of a block per thread");
static_assert(kMaxFrames * 16 <= kBlock && kMaxFrames <= 32, "frame table: one load per thread");

// first .. last block index on one axis of the points q - rho .. q + rho, cut to the table; false: none in the table
__device__ __forceinline__ bool block_range(float q, float rho, float lower, float block_size, uint32_t tb, uint32_t& b0, uint32_t& b1) {
    const float lo = floorf(((q - rho) - lower) / block_size);
    const float hi = floorf(((q + rho) - lower) / block_size);
    if (!(hi >= 0.f && lo < (float)tb)) return false;  // a NaN fails
    b0 = (uint32_t)fmaxf(lo, 0.f);
    b1 = (uint32_t)fminf(hi, (float)(tb - 1u));
    return true;
}

__global__ void __launch_bounds__(kBlock) k_tsdf_blocks_touch(const nvo_tsdf_blocks_args a) {
    __shared__ float cam[kMaxFrames * 16], pose[kMaxFrames * 16];
    if (threadIdx.x < a.K * 16u) {
        cam[threadIdx.x] = a.frames[threadIdx.x];
        pose[threadIdx.x] = a.touch_frames[threadIdx.x];
    }
    __syncthreads();
    const uint64_t n_pix = (uint64_t)a.H * a.W, total = n_pix * a.K;
    const float h = a.voxel_size * 0.5f, quarter = a.voxel_size * 0.25f, block_size = a.voxel_size * 8.f;  // exact
    for (uint64_t g = (uint64_t)blockIdx.x * kBlock + threadIdx.x; g < total; g += (uint64_t)gridDim.x * kBlock) {
        const float d = a.depth[g];
        if (!(d > 0.f && d <= a.depth_max)) continue;  // a NaN fails
        const uint32_t f = (uint32_t)(g / n_pix), r = (uint32_t)(g % n_pix);
        const uint32_t vi = r / a.W, ui = r % a.W;
        const float* c = cam + 16 * f;
        const float* m = pose + 16 * f;
        const float ca = ((float)ui - c[14]) / c[12], cb = ((float)vi - c[15]) / c[13];
        const float slant = sqrtf((ca * ca + cb * cb) + 1.f);
        const float z_lo = fmaxf(d - a.trunc, 0.f), z_hi = d + a.trunc;
        const uint32_t bit = 1u << f;
        uint32_t px0 = ~0u, px1 = 0, py0 = 0, py1 = 0, pz0 = 0, pz1 = 0;  // the previous sample's ranges
        for (uint32_t n = 0; n < a.n_samples; ++n) {
            const float z = fminf(z_lo + (float)n * h, z_hi);
            const float xc = ca * z, yc = cb * z;
            const float px = m[0] * xc + m[1] * yc + m[2] * z + m[3];
            const float py = m[4] * xc + m[5] * yc + m[6] * z + m[7];
            const float pz = m[8] * xc + m[9] * yc + m[10] * z + m[11];
            const float rho = (z * m[12] + quarter * slant) + quarter;
            uint32_t x0, x1, y0, y1, z0, z1;
            const bool in = block_range(px, rho, a.lower_x, block_size, a.tbx, x0, x1) &&
                            block_range(py, rho, a.lower_y, block_size, a.tby, y0, y1) &&
                            block_range(pz, rho, a.lower_z, block_size, a.tbz, z0, z1);
            if (in && !(x0 == px0 && x1 == px1 && y0 == py0 && y1 == py1 && z0 == pz0 && z1 == pz1)) {
                for (uint32_t bi = x0; bi <= x1; ++bi)
                    for (uint32_t bj = y0; bj <= y1; ++bj)
                        for (uint32_t bk = z0; bk <= z1; ++bk) {  // bi < tbx, bj < tby, bk < tbz by block_range
                            uint32_t* w = a.marks + ((size_t)bi * a.tby + bj) * a.tbz + bk;
                            if (!(*w & bit)) atomicOr(w, bit);  // (the plain read only saves atomics: a stale 0 repeats one)
                        }
                px0 = x0, px1 = x1, py0 = y0, py1 = y1, pz0 = z0, pz1 = z1;
            }
            if (z >= z_hi) break;  // every further sample is this one
        }
    }
}

__global__ void __launch_bounds__(kBlock) k_tsdf_blocks_integrate(const nvo_tsdf_blocks_args a, uint32_t n_table) {
    __shared__ float cam[kMaxFrames * 16];
    if (threadIdx.x < a.K * 16u) cam[threadIdx.x] = a.frames[threadIdx.x];
    __syncthreads();
    const float fW = (float)a.W, fH = (float)a.H;
    const uint32_t in_launch = a.K >= 32u ? ~0u : ((1u << a.K) - 1u);
    for (uint32_t e = blockIdx.x; e < a.n_list; e += gridDim.x) {
        // ---- the block of this entry (workgroup-uniform) ----
        const int32_t tix = a.list[e];
        if (tix < 0 || (uint32_t)tix >= n_table) continue;
        const int32_t id = a.table[tix];
        if (id < 0 || (uint32_t)id >= a.n_allocated) continue;
        const uint32_t live = a.list_mask[e] & in_launch;
        if (live == 0u) continue;
        const uint32_t bk = (uint32_t)tix % a.tbz, bij = (uint32_t)tix / a.tbz, bj = bij % a.tby, bi = bij / a.tby;
#pragma unroll
        for (uint32_t half = 0; half < 2; ++half) {
            const uint32_t local = threadIdx.x + half * kBlock;  // (li*8 + lj)*8 + lk
            const uint32_t i = bi * kB + (local >> 6), j = bj * kB + ((local >> 3) & 7u), k = bk * kB + (local & 7u);
            const size_t idx = (size_t)id * kBlockVoxels + local;              // < 2^31: n_allocated <= 2^22
            const size_t cidx = (size_t)id * (3 * kBlockVoxels) + local;
            const float px = a.lower_x + (float)i * a.voxel_size;
            const float py = a.lower_y + (float)j * a.voxel_size;
            const float pz = a.lower_z + (float)k * a.voxel_size;
            tsdf_fuse_voxel(cam, a.K, live, a.H, a.W, fW, fH, a.depth, a.rgb, a.trunc, a.depth_max, px, py, pz, a.tsdf,
                            a.weight, a.color, idx, cidx, kBlockVoxels);
        }
    }
}

int blocks_check(const nvo_tsdf_blocks_args& a, const char* what, uint64_t* n_table) {
    NVO_REQUIRE(a.frames && a.depth, "%s: NULL frames or depth", what);
    if (int rc = tsdf_table_check(what, a.tbx, a.tby, a.tbz, n_table)) return rc;
    return tsdf_frames_check(what, a.K, a.H, a.W, a.voxel_size, a.trunc);
}

}  // namespace

extern "C" {

int nvo_tsdf_blocks_touch(nvo_stream_t stream, const nvo_tsdf_blocks_args* args) {
    NVO_REQUIRE(args != nullptr, "tsdf_blocks_touch: args is NULL");
    const nvo_tsdf_blocks_args a = *args;
    uint64_t n_table;
    if (int rc = blocks_check(a, "tsdf_blocks_touch", &n_table)) return rc;
    NVO_REQUIRE(a.touch_frames && a.marks, "tsdf_blocks_touch: NULL touch_frames or marks");
    NVO_REQUIRE(a.n_samples >= 1 && a.n_samples <= kMaxSamples, "tsdf_blocks_touch: %u samples per pixel not in 1..%u", a.n_samples,
                kMaxSamples);
    const uint64_t total = (uint64_t)a.H * a.W * a.K;
    const uint64_t want = (total + kBlock - 1) / kBlock;
    const uint32_t grid = (uint32_t)(want < kMaxGrid ? want : kMaxGrid);
    NVO_PROF(stream, "tsdf_blocks_touch");
    NVO_LAUNCH(k_tsdf_blocks_touch, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, a);
    NVO_CHECK_LAUNCH();
    return NVO_OK;
}

int nvo_tsdf_blocks_integrate(nvo_stream_t stream, const nvo_tsdf_blocks_args* args) {
    NVO_REQUIRE(args != nullptr, "tsdf_blocks_integrate: args is NULL");
    const nvo_tsdf_blocks_args a = *args;
    uint64_t n_table;
    if (int rc = blocks_check(a, "tsdf_blocks_integrate", &n_table)) return rc;
    NVO_REQUIRE(a.n_allocated <= NVO_TSDF_BLOCKS_MAX_ALLOCATED,
                "tsdf_blocks_integrate: %u allocated blocks, more than %u (block id * 512 + local index must stay below 2^31)",
                a.n_allocated, NVO_TSDF_BLOCKS_MAX_ALLOCATED);
    NVO_REQUIRE(a.n_list <= n_table, "tsdf_blocks_integrate: a list of %u blocks for a table of %llu", a.n_list,
                (unsigned long long)n_table);
    if (a.n_list == 0 || a.n_allocated == 0) return NVO_OK;
    NVO_REQUIRE(a.table && a.tsdf && a.weight && a.color && a.rgb && a.list && a.list_mask, "tsdf_blocks_integrate: NULL argument");
    NVO_PROF(stream, "tsdf_blocks_integrate");
    NVO_LAUNCH(k_tsdf_blocks_integrate, dim3(a.n_list), dim3(kBlock), 0, (hipStream_t)stream, a, (uint32_t)n_table);
    NVO_CHECK_LAUNCH();
    return NVO_OK;
}

}  // extern "C"
