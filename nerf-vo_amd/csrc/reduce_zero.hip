// Helpers every other translation unit calls: clearing device ranges (one range, or a plan of several in one launch),
// the deterministic reductions (EngineConfig.deterministic: fixed summation orders instead of float atomics) and the
// fold of the weight-gradient replicas a fused-MLP backward spreads its adds over.
#include "nvo_kernels.h"
#include "../../include/nerfvo_hip.h"

#include <string.h>

namespace {

__global__ void __launch_bounds__(256)
k_zero_u32(uint32_t* __restrict__ p, uint64_t n) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) p[i] = 0u;
}

// several device ranges cleared by ONE launch (a training step's accumulate-into buffers); plan: nvo_common.h
__global__ void __launch_bounds__(256)
k_zero_ranges(NvoZeroPlan r) {
    nvo_zero_plan_block(r, blockIdx.x);
}

// ---- deterministic reductions (EngineConfig.deterministic): fixed summation orders instead of float atomics ----
__global__ void __launch_bounds__(256)
k_reduce_partials(const float* __restrict__ partial, uint32_t n_blocks, uint64_t n, float* __restrict__ dst) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    float acc = 0.f;
    for (uint32_t b = 0; b < n_blocks; ++b) acc += partial[(uint64_t)b * n + e];
    dst[e] += acc;
}

__global__ void __launch_bounds__(256)
k_reduce_by_camera(uint32_t R, uint32_t K, const float* __restrict__ rows, uint32_t row_stride, const void* __restrict__ cam,
                   int cam_i64x3, float* __restrict__ out) {
    // one workgroup per camera: 8 sub-sequences (rays r = s, s + 8, ...) of 32 lanes (columns), each summed in ray
    // order, then combined s = 0..7 -- every order is fixed, so the result does not depend on scheduling
    __shared__ float part[8][32];
    const uint32_t c = blockIdx.x, k = threadIdx.x & 31u, sub = threadIdx.x >> 5;
    float acc = 0.f;
    for (uint32_t r = sub; r < R; r += 8u) {
        const int64_t cr = cam_i64x3 ? reinterpret_cast<const int64_t*>(cam)[3 * (size_t)r]
                                     : (int64_t)reinterpret_cast<const int32_t*>(cam)[r];
        if (cr == (int64_t)c && k < K) acc += rows[(size_t)r * row_stride + k];
    }
    part[sub][k] = acc;
    __syncthreads();
    if (sub == 0 && k < K) {
        float t = 0.f;
#pragma unroll
        for (int q = 0; q < 8; ++q) t += part[q][k];
        out[(size_t)c * K + k] += t;
    }
}

__global__ void __launch_bounds__(256)
k_color_tiles_to_rays(uint32_t R, uint32_t tiles_per_ray, const float* __restrict__ tile_partial,
                      float* __restrict__ per_ray, float* __restrict__ d_sh) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= R * 48u) return;
    const uint32_t r = i / 48u, k = i % 48u;
    float acc = 0.f;
    for (uint32_t t = 0; t < tiles_per_ray; ++t) acc += tile_partial[((size_t)r * tiles_per_ray + t) * 48u + k];
    per_ray[i] = acc;
    if (d_sh && k >= 32u) d_sh[(size_t)r * 16u + (k - 32u)] += acc;
}

struct FoldEntries {
    uint32_t n_entries;
    float* rep[8];
    float* dst[8];
    uint32_t n_rep[8];
    uint64_t n[8], first[9];  // first[i]: index of entry i's first element in the launch's flat index space
};
__global__ void __launch_bounds__(256)
k_fold_replicas(FoldEntries f) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= f.first[f.n_entries]) return;
    uint32_t k = 0;
    while (k + 1 < f.n_entries && i >= f.first[k + 1]) ++k;
    const uint64_t e = i - f.first[k];
    // (all copies requested before the first is used: one memory round trip; fixed summation order -- the copies
    // themselves were filled by float atomics)
    float acc = f.dst[k][e];
    for (uint32_t r0 = 0; r0 < f.n_rep[k]; r0 += 8u) {
        float v[8];
#pragma unroll
        for (uint32_t q = 0; q < 8u; ++q) v[q] = r0 + q < f.n_rep[k] ? f.rep[k][(size_t)(r0 + q) * f.n[k] + e] : 0.f;
#pragma unroll
        for (uint32_t q = 0; q < 8u; ++q) {
            acc += v[q];
            if (r0 + q < f.n_rep[k]) f.rep[k][(size_t)(r0 + q) * f.n[k] + e] = 0.f;
        }
    }
    f.dst[k][e] = acc;
}

}  // namespace

int nvo_reduce_partials(hipStream_t stream, const float* partial, uint32_t n_blocks, uint64_t n, float* dst) {
    NVO_REQUIRE(partial && dst, "reduce_partials: NULL argument");
    if (n == 0 || n_blocks == 0) return NVO_OK;
    NVO_PROF(stream, "reduce_partials");
    NVO_LAUNCH(k_reduce_partials, dim3(nvo_div_up(n, 256)), dim3(256), 0, stream, partial, n_blocks, n, dst);
    NVO_CHECK_LAUNCH();
    return NVO_OK;
}

int nvo_reduce_by_camera(hipStream_t stream, uint32_t R, uint32_t K, const float* rows, uint32_t row_stride,
                         const void* cam, int cam_i64x3, uint32_t F, float* out) {
    NVO_REQUIRE(rows && cam && out && K >= 1 && K <= 32, "reduce_by_camera: bad argument (K <= 32)");
    if (R == 0 || F == 0) return NVO_OK;
    NVO_PROF(stream, "reduce_by_camera");
    NVO_LAUNCH(k_reduce_by_camera, dim3(F), dim3(256), 0, stream, R, K, rows, row_stride, cam, cam_i64x3, out);
    NVO_CHECK_LAUNCH();
    return NVO_OK;
}

int nvo_color_tiles_to_rays(hipStream_t stream, uint32_t R, uint32_t tiles_per_ray, const float* tile_partial,
                            float* per_ray, float* d_sh) {
    NVO_REQUIRE(tile_partial && per_ray && tiles_per_ray >= 1, "color_tiles_to_rays: bad argument");
    if (R == 0) return NVO_OK;
    NVO_LAUNCH(k_color_tiles_to_rays, dim3(nvo_div_up((uint64_t)R * 48, 256)), dim3(256), 0, stream, R, tiles_per_ray,
               tile_partial, per_ray, d_sh);
    NVO_CHECK_LAUNCH();
    return NVO_OK;
}

int nvo_zero_async(void* ptr, size_t bytes, hipStream_t stream) {
    NVO_REQUIRE((bytes & 3u) == 0 && ((uintptr_t)ptr & 3u) == 0, "zero_async: %zu bytes not 4-byte granular", bytes);
    if (bytes == 0) return NVO_OK;
    const uint64_t n = bytes / 4;
    uint32_t blocks = nvo_div_up(n, 256 * 8);
    if (blocks > 2048) blocks = 2048;
    NVO_LAUNCH(k_zero_u32, dim3(blocks), dim3(256), 0, stream, (uint32_t*)ptr, n);
    NVO_CHECK_LAUNCH();
    return NVO_OK;
}

int nvo_zero_plan_build(uint32_t n_ranges, void* const* ptrs, const uint64_t* bytes, NvoZeroPlan* plan) {
    if (n_ranges > kZeroMaxRanges) {
        nvo_set_error("zero_ranges: at most %u ranges (got %u)", kZeroMaxRanges, n_ranges);
        return -1;
    }
    if (n_ranges != 0 && !(ptrs && bytes)) {
        nvo_set_error("zero_ranges: NULL argument");
        return -1;
    }
    NvoZeroPlan& r = *plan;
    memset(&r, 0, sizeof(r));
    uint32_t k = 0, blocks_total = 0;
    for (uint32_t i = 0; i < n_ranges; ++i) {
        if (bytes[i] == 0) continue;
        if (!(ptrs[i] && (bytes[i] & 3u) == 0 && ((uintptr_t)ptrs[i] & 3u) == 0)) {
            nvo_set_error("zero_ranges: range %u is not 4-byte granular", i);
            return -1;
        }
        r.ptr[k] = (uint32_t*)ptrs[i];
        r.words[k] = bytes[i] / 4;
        uint32_t b = nvo_div_up(r.words[k], (uint64_t)256 * 16);  // 16 dwords per thread and pass
        if (b < 1) b = 1;
        if (b > 512) b = 512;
        r.first_block[k] = blocks_total;
        blocks_total += b;
        ++k;
    }
    r.n = k;
    for (uint32_t i = k; i <= kZeroMaxRanges; ++i) r.first_block[i] = blocks_total;
    return (int)blocks_total;
}

extern "C" {

int nvo_zero_ranges(nvo_stream_t stream, uint32_t n_ranges, void* const* ptrs, const uint64_t* bytes) {
    NvoZeroPlan r;
    const int blocks_total = nvo_zero_plan_build(n_ranges, ptrs, bytes, &r);
    if (blocks_total < 0) return NVO_ERR_INVALID;
    if (blocks_total == 0) return NVO_OK;
    NVO_PROF(stream, "zero_ranges");
    NVO_LAUNCH(k_zero_ranges, dim3((uint32_t)blocks_total), dim3(256), 0, (hipStream_t)stream, r);
    NVO_CHECK_LAUNCH();
    return NVO_OK;
}

int nvo_fold_replicas(nvo_stream_t stream, uint32_t n_entries, float* const* replicas, const uint32_t* n_replicas,
                      const uint64_t* n, float* const* dst) {
    NVO_REQUIRE(n_entries >= 1 && n_entries <= 8 && replicas && n_replicas && n && dst, "fold_replicas: 1..8 entries");
    FoldEntries f;
    memset(&f, 0, sizeof(f));
    uint64_t total = 0;
    for (uint32_t i = 0; i < n_entries; ++i) {
        NVO_REQUIRE(replicas[i] && dst[i], "fold_replicas: NULL buffer");
        f.rep[f.n_entries] = replicas[i];
        f.dst[f.n_entries] = dst[i];
        f.n_rep[f.n_entries] = n_replicas[i];
        f.n[f.n_entries] = n[i];
        f.first[f.n_entries] = total;
        total += n[i];
        ++f.n_entries;
    }
    f.first[f.n_entries] = total;
    if (total == 0) return NVO_OK;
    NVO_PROF(stream, "fold_replicas");
    NVO_LAUNCH(k_fold_replicas, dim3((uint32_t)nvo_div_up(total, 256)), dim3(256), 0, (hipStream_t)stream, f);
    NVO_CHECK_LAUNCH();
    return NVO_OK;
}

}  // extern "C"
