// TSDF fusion of depth + colour frames into a dense volume (DESIGN.md "TSDF fusion"): the integration step behind
// EvaluationRenderer.render_mesh.  The reference fuses with Open3D's VoxelBlockGrid on the CPU; here the volume is a
// dense box, one thread owns one voxel for the whole launch and applies the K frames of the launch in table order by
// the per-voxel rule of tsdf_dev.h (tsdf_fuse_voxel, stated there).  The voxel's five values live in registers across the
// K frames, are loaded when the first frame touches them and stored once: the result is bitwise independent of how a
// frame sequence is cut into launches, and the volume is read and written at most once per launch.
//
// Work decomposition: a 256-thread workgroup owns a brick of 2 x 4 x 32 voxels (z fastest: every wave reads two runs
// of 32 floats = 128 bytes per plane) and grid-strides over the bricks.  Per brick and frame, each wave first decides
// from the brick's eight corner samples whether the frame can touch the brick at all (lane = frame * 8 + corner, six
// ballots per eight frames).  A frame is dropped only when
//   * every corner has zc <= -voxel_size, or
//   * every corner has zc >= voxel_size and all of them fall off the same image side by more than one pixel beyond
//     the rounding limit (u < -1.5, u > W + 0.5, likewise v).
// Both are conservative for the per-voxel rule above: the voxels of a brick lie inside the box of its corner samples,
// zc is affine in p and, with every zc positive, u and v of a voxel lie in the hull of the corners' u and v.  The
// voxel_size / one-pixel margins absorb the fp32 rounding of the per-voxel evaluation: zc of a voxel is off by a few
// ulp of the world coordinates, far less than a voxel as long as those stay below some 2^18 voxel sizes (4 km at 1/64),
// and at zc >= voxel_size the rounding of u, v stays well below the pixel of margin (focal length x coordinate ulp /
// voxel_size: 0.04 pixel for fx = 600, coordinates of a few metres, voxel 1/64).  Bricks that straddle the camera plane
// are never culled.
#include "nvo_kernels.h"
#include "tsdf_dev.h"

namespace {

constexpr int kBlock = 256;
constexpr uint32_t kBX = 2, kBY = 4, kBZ = 32;  // brick, z fastest; kBX * kBY * kBZ == kBlock
constexpr uint32_t kMaxGrid = 2048;             // 256 CUs x 8 workgroups, grid-stride beyond
constexpr uint32_t kMaxFrames = NVO_TSDF_MAX_FRAMES;
static_assert(kBX * kBY * kBZ == kBlock, "one thread per voxel of a brick");
static_assert(kMaxFrames * 16 <= kBlock && kMaxFrames <= 32 && kMaxFrames % 8 == 0, "frame table: one load per thread");

// bit g is set when all eight lanes of group g (lanes 8g .. 8g+7) are set in m
__device__ __forceinline__ uint32_t groups_all(unsigned long long m) {
    m &= m >> 4;
    m &= m >> 2;
    m &= m >> 1;  // bit 8g = AND of the byte
    uint32_t out = 0;
#pragma unroll
    for (uint32_t g = 0; g < 8; ++g) out |= (uint32_t)((m >> (8 * g)) & 1ull) << g;
    return out;
}

__global__ void __launch_bounds__(kBlock)
k_tsdf_integrate(const nvo_tsdf_args a, uint32_t nby, uint32_t nbz, uint64_t n_bricks) {
    __shared__ float cam[kMaxFrames * 16];
    if (threadIdx.x < a.K * 16u) cam[threadIdx.x] = a.frames[threadIdx.x];
    __syncthreads();

    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t tz = threadIdx.x % kBZ, ty = (threadIdx.x / kBZ) % kBY, tx = threadIdx.x / (kBZ * kBY);
    const size_t n_vox = (size_t)a.nx * a.ny * a.nz;
    const float fW = (float)a.W, fH = (float)a.H;

    for (uint64_t b = blockIdx.x; b < n_bricks; b += gridDim.x) {
        const uint32_t bz = (uint32_t)(b % nbz);
        const uint64_t bxy = b / nbz;
        const uint32_t by = (uint32_t)(bxy % nby), bx = (uint32_t)(bxy / nby);
        const uint32_t i0 = bx * kBX, j0 = by * kBY, k0 = bz * kBZ;

        // ---- which frames can touch the brick (wave-uniform) ----
        uint32_t live = 0;
        {
            // corner sample of this lane: the first / last voxel of the brick that lies inside the volume
            const uint32_t ci = (lane & 1u) ? min(i0 + kBX - 1u, a.nx - 1u) : i0;
            const uint32_t cj = (lane & 2u) ? min(j0 + kBY - 1u, a.ny - 1u) : j0;
            const uint32_t ck = (lane & 4u) ? min(k0 + kBZ - 1u, a.nz - 1u) : k0;
            const float px = a.lower_x + (float)ci * a.voxel_size;
            const float py = a.lower_y + (float)cj * a.voxel_size;
            const float pz = a.lower_z + (float)ck * a.voxel_size;
            for (uint32_t f0 = 0; f0 < a.K; f0 += 8) {
                const uint32_t f = min(f0 + (lane >> 3), a.K - 1u);  // lanes past the batch repeat its last frame
                const float* c = cam + 16 * f;
                const float xc = c[0] * px + c[1] * py + c[2] * pz + c[3];
                const float yc = c[4] * px + c[5] * py + c[6] * pz + c[7];
                const float zc = c[8] * px + c[9] * py + c[10] * pz + c[11];
                const bool front = zc >= a.voxel_size;
                const float u = c[12] * xc / zc + c[14], v = c[13] * yc / zc + c[15];
                const uint32_t behind = groups_all(__ballot(zc <= -a.voxel_size));
                const uint32_t off = groups_all(__ballot(front && u < -1.5f)) | groups_all(__ballot(front && u > fW + 0.5f)) |
                                     groups_all(__ballot(front && v < -1.5f)) | groups_all(__ballot(front && v > fH + 0.5f));
                const uint32_t in_batch = (a.K - f0 >= 8u) ? 0xFFu : ((1u << (a.K - f0)) - 1u);
                live |= (~(behind | off) & in_batch) << f0;
            }
            live = (uint32_t)__builtin_amdgcn_readfirstlane((int)live);
        }

        const uint32_t i = i0 + tx, j = j0 + ty, k = k0 + tz;
        if (live != 0u && i < a.nx && j < a.ny && k < a.nz) {  // partial bricks at the upper faces: predication
            const size_t idx = ((size_t)i * a.ny + j) * a.nz + k;
            const float px = a.lower_x + (float)i * a.voxel_size;
            const float py = a.lower_y + (float)j * a.voxel_size;
            const float pz = a.lower_z + (float)k * a.voxel_size;
            tsdf_fuse_voxel(cam, a.K, live, a.H, a.W, fW, fH, a.depth, a.rgb, a.trunc, a.depth_max, px, py, pz, a.tsdf,
                            a.weight, a.color, idx, idx, n_vox);
        }
    }
}

}  // namespace

extern "C" {

int nvo_tsdf_integrate(nvo_stream_t stream, const nvo_tsdf_args* args) {
    NVO_REQUIRE(args != nullptr, "tsdf_integrate: args is NULL");
    const nvo_tsdf_args a = *args;
    NVO_REQUIRE(a.tsdf && a.weight && a.color && a.frames && a.depth && a.rgb, "tsdf_integrate: NULL argument");
    NVO_REQUIRE(a.nx >= 1 && a.ny >= 1 && a.nz >= 1 && a.nx < (1u << 31) && a.ny < (1u << 31) && a.nz < (1u << 31) &&
                    (uint64_t)a.nx * a.ny < (1ull << 31) && (uint64_t)a.nx * a.ny * a.nz < (1ull << 31),
                "tsdf_integrate: volume %u x %u x %u must have between 1 and 2^31 - 1 voxels", a.nx, a.ny, a.nz);
    if (int rc = tsdf_frames_check("tsdf_integrate", a.K, a.H, a.W, a.voxel_size, a.trunc)) return rc;
    const uint32_t nbx = nvo_div_up(a.nx, kBX), nby = nvo_div_up(a.ny, kBY), nbz = nvo_div_up(a.nz, kBZ);
    const uint64_t n_bricks = (uint64_t)nbx * nby * nbz;
    const uint32_t grid = (uint32_t)(n_bricks < kMaxGrid ? n_bricks : kMaxGrid);
    NVO_PROF(stream, "tsdf_integrate");
    NVO_LAUNCH(k_tsdf_integrate, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, a, nby, nbz, n_bricks);
    NVO_CHECK_LAUNCH();
    return NVO_OK;
}

}  // extern "C"
