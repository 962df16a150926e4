// 2-D evaluation metrics of batches of frames (include/nerfvo_hip.h section N): the accumulators
// behind metrics_2d_*.csv.  Kernels:
//
//   k_m2d_color<FLOAT>   a workgroup owns one 32 x 32 tile of one channel of one frame.  It stages the tile plus a 5-pixel
//                        halo of both images in LDS as fp32 (zero outside the image: a tap there adds taps[t] * 0 = +0 and
//                        leaves the running sum as it was, i.e. the tap is skipped), writes the five horizontal moments
//                        (a, b, a*a, b*b, a*b) of the 42 staged rows to LDS, runs the vertical pass, forms the SSIM map
//                        and sums llrint(double(s) * 2^32) as an integer.  The uint8 form also sums the two squared
//                        differences of the tile's own pixels while it stages them.  Each workgroup stores its three
//                        integers in its own slot; k_m2d_color_fold adds the slots of a (frame, channel).  Integer sums:
//                        no order.  fp32 with one rounding per written operation (-ffp-contract=off, correctly rounded
//                        division): tests/helpers/metrics2d_oracle.py gives the same integers.
//   k_m2d_depth<PASS>    float64.  A frame is cut into G = nvo_m2d_depth_chunks(H, W) contiguous chunks, one workgroup
//                        each; thread t sums the pixels first + t, first + t + 256, ... in that order, the 256 partial sums
//                        fold as a binary tree in LDS, the workgroup's sums go to its own slot.  Pass 1: n, sum gt, sum
//                        pred.  Pass 2 folds the slots of pass 1 in ascending order (every workgroup for itself, thread 0),
//                        forms the scale and sums the five errors and the three counts.  k_m2d_depth_fold adds the slots of
//                        pass 2 in ascending order.  The order depends on (H, W) alone.
//
// Bounds: the launchers check pointers, sizes and the products that index; every pixel a kernel touches is compared
// against H and W first; every slot index is < the slot count the scratch size was computed from.
#include "nvo_kernels.h"
#include "../../include/nerfvo_hip.h"

#include <math.h>

namespace {

constexpr int kBlock = 256;
constexpr int kTH = NVO_M2D_TILE_H, kTW = NVO_M2D_TILE_W, kTaps = NVO_M2D_TAPS, kR = kTaps / 2;
constexpr int kSH = kTH + 2 * kR, kSW = kTW + 2 * kR;  // staged rows and columns: 42 x 42
constexpr int kSWp = kSW + 1;                          // row pitch 43: the horizontal pass's 8 x 4 lanes hit distinct banks
constexpr int kSpan = 4 + kTaps - 1;                   // inputs of four neighbouring outputs: 14
static_assert(kTH == 32 && kTW == 32 && kBlock == 256, "vertical pass: a thread owns 4 rows of one column");
static_assert(kTaps == 11, "window");

struct TapArgs {
    float g[kTaps];
};

template <bool FLOAT>
__global__ void __launch_bounds__(kBlock) k_m2d_color(const void* __restrict__ pa, const void* __restrict__ pb,
                                                      unsigned long long* __restrict__ slots, uint32_t H, uint32_t W,
                                                      uint32_t tiles_x, uint32_t tiles, const TapArgs taps) {
    __shared__ float sa[kSH][kSWp], sb[kSH][kSWp];
    __shared__ float mom[5][kSH][kTW];
    __shared__ unsigned long long red[NVO_M2D_COLOR_WORDS];
    const uint32_t tid = threadIdx.x, tile = blockIdx.x, fc = blockIdx.y, f = fc / 3u, c = fc % 3u;
    const int row0 = (int)((tile / tiles_x) * kTH) - kR, col0 = (int)((tile % tiles_x) * kTW) - kR;
    if (tid < NVO_M2D_COLOR_WORDS) red[tid] = 0ull;

    // ---- stage the tile and its halo ----
    uint32_t wrap = 0, tru = 0;  // at most 7 pixels per thread: 7 * 255^2 fits
    for (int i = (int)tid; i < kSH * kSW; i += kBlock) {
        const int r = i / kSW, q = i % kSW, y = row0 + r, x = col0 + q;
        float va = 0.f, vb = 0.f;
        if (y >= 0 && y < (int)H && x >= 0 && x < (int)W) {
            if (FLOAT) {
                const size_t idx = ((size_t)fc * H + (uint32_t)y) * W + (uint32_t)x;
                va = ((const float*)pa)[idx];
                vb = ((const float*)pb)[idx];
            } else {
                const size_t idx = (((size_t)f * H + (uint32_t)y) * W + (uint32_t)x) * 3u + c;
                const uint8_t ua = ((const uint8_t*)pa)[idx], ub = ((const uint8_t*)pb)[idx];
                va = ((float)ua / 255.0f) * 2.0f - 1.0f;
                vb = ((float)ub / 255.0f) * 2.0f - 1.0f;
                if (r >= kR && r < kR + kTH && q >= kR && q < kR + kTW) {  // the tile's own pixel
                    const uint8_t d = (uint8_t)(ua - ub);
                    wrap += (uint8_t)(d * d);
                    const int dd = (int)ua - (int)ub;
                    tru += (uint32_t)(dd * dd);
                }
            }
        }
        sa[r][q] = va;
        sb[r][q] = vb;
    }
    __syncthreads();

    // ---- horizontal pass: four neighbouring columns of one staged row per item ----
    for (int it = (int)tid; it < kSH * (kTW / 4); it += kBlock) {
        const int r = it / (kTW / 4), q0 = (it % (kTW / 4)) * 4;
        float xa[kSpan], xb[kSpan];
#pragma unroll
        for (int k = 0; k < kSpan; ++k) {
            xa[k] = sa[r][q0 + k];
            xb[k] = sb[r][q0 + k];
        }
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            float m0 = 0.f, m1 = 0.f, m2 = 0.f, m3 = 0.f, m4 = 0.f;
#pragma unroll
            for (int t = 0; t < kTaps; ++t) {
                const float g = taps.g[t], u = xa[o + t], v = xb[o + t];
                m0 = m0 + g * u;
                m1 = m1 + g * v;
                m2 = m2 + g * (u * u);
                m3 = m3 + g * (v * v);
                m4 = m4 + g * (u * v);
            }
            mom[0][r][q0 + o] = m0;
            mom[1][r][q0 + o] = m1;
            mom[2][r][q0 + o] = m2;
            mom[3][r][q0 + o] = m3;
            mom[4][r][q0 + o] = m4;
        }
    }
    __syncthreads();

    // ---- vertical pass, SSIM map and the tile's sum: four rows of one column per thread ----
    const int q = (int)(tid % kTW), r0 = (int)(tid / kTW) * 4;
    float out[5][4];
#pragma unroll
    for (int p = 0; p < 5; ++p) {
        float v[kSpan];
#pragma unroll
        for (int k = 0; k < kSpan; ++k) v[k] = mom[p][r0 + k][q];
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            float acc = 0.f;
#pragma unroll
            for (int t = 0; t < kTaps; ++t) acc = acc + taps.g[t] * v[o + t];
            out[p][o] = acc;
        }
    }
    const float C1 = 0.0001f, C2 = 0.0009f;  // float32(0.01^2), float32(0.03^2)
    long long fixed = 0;
    const int x = col0 + kR + q;
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        const int y = row0 + kR + r0 + o;
        if (y < (int)H && x < (int)W) {
            const float ma = out[0][o], mb = out[1][o], saa = out[2][o], sbb = out[3][o], sab = out[4][o];
            const float maa = ma * ma, mbb = mb * mb, mab = ma * mb;
            const float va = saa - maa, vb = sbb - mbb, cab = sab - mab;
            const float num = (2.0f * mab + C1) * (2.0f * cab + C2);
            const float den = ((maa + mbb) + C1) * ((va + vb) + C2);
            const float s = num / den;
            fixed += llrint((double)s * 4294967296.0);
        }
    }
    atomicAdd(&red[0], (unsigned long long)wrap);  // LDS integer atomics: no order to speak of
    atomicAdd(&red[1], (unsigned long long)tru);
    atomicAdd(&red[2], (unsigned long long)fixed);
    __syncthreads();
    if (tid < NVO_M2D_COLOR_WORDS) slots[((size_t)fc * tiles + tile) * NVO_M2D_COLOR_WORDS + tid] = red[tid];
}

__global__ void __launch_bounds__(kBlock) k_m2d_color_fold(const unsigned long long* __restrict__ slots,
                                                           unsigned long long* __restrict__ table, uint32_t tiles) {
    __shared__ unsigned long long red[NVO_M2D_COLOR_WORDS];
    const uint32_t fc = blockIdx.x;
    if (threadIdx.x < NVO_M2D_COLOR_WORDS) red[threadIdx.x] = 0ull;
    __syncthreads();
    unsigned long long s[NVO_M2D_COLOR_WORDS] = {};
    for (uint32_t t = threadIdx.x; t < tiles; t += kBlock)
#pragma unroll
        for (int w = 0; w < NVO_M2D_COLOR_WORDS; ++w) s[w] += slots[((size_t)fc * tiles + t) * NVO_M2D_COLOR_WORDS + w];
#pragma unroll
    for (int w = 0; w < NVO_M2D_COLOR_WORDS; ++w) atomicAdd(&red[w], s[w]);
    __syncthreads();
    if (threadIdx.x < NVO_M2D_COLOR_WORDS) table[(size_t)fc * NVO_M2D_COLOR_WORDS + threadIdx.x] = red[threadIdx.x];
}

// ---------------------------------------------------------------------------------------------------------------
// depth
// ---------------------------------------------------------------------------------------------------------------
constexpr uint32_t kDepthMaxChunks = 256, kDepthChunkTarget = 2048;
constexpr int kP1 = 3, kP2 = 8;  // sums per workgroup of pass 1 and of pass 2

__host__ __device__ inline uint32_t depth_chunks(uint64_t n_pix) {
    const uint64_t want = (n_pix + kDepthChunkTarget - 1) / kDepthChunkTarget;
    return (uint32_t)(want < 1 ? 1 : (want > kDepthMaxChunks ? kDepthMaxChunks : want));
}

__device__ __forceinline__ double depth_load(const void* p, size_t i, bool f64) {
    return f64 ? ((const double*)p)[i] : (double)((const float*)p)[i];
}

// v[0 .. N) of every thread -> the tree sums in buf[0 .. N)[0]
template <int N>
__device__ __forceinline__ void tree_fold(double (&v)[N], double (*buf)[kBlock]) {
    const uint32_t t = threadIdx.x;
#pragma unroll
    for (int k = 0; k < N; ++k) buf[k][t] = v[k];
    __syncthreads();
    for (uint32_t s = kBlock / 2; s >= 1; s >>= 1) {
        if (t < s)
#pragma unroll
            for (int k = 0; k < N; ++k) buf[k][t] = buf[k][t] + buf[k][t + s];
        __syncthreads();
    }
}

template <int PASS>
__global__ void __launch_bounds__(kBlock) k_m2d_depth(const nvo_m2d_depth_args a, double* __restrict__ p1, double* __restrict__ p2,
                                                      uint32_t G, uint32_t chunk) {
    __shared__ double buf[PASS == 1 ? kP1 : kP2][kBlock];
    __shared__ double scale_s;
    const uint32_t g = blockIdx.x, f = blockIdx.y, t = threadIdx.x;
    const uint64_t n_pix = (uint64_t)a.H * a.W;
    const uint64_t first = (uint64_t)g * chunk, last = first + chunk < n_pix ? first + chunk : n_pix;
    const size_t base = (size_t)f * n_pix;
    const bool gt64 = a.gt_f64 != 0, pr64 = a.pred_f64 != 0;
    if (PASS == 1) {
        double v[kP1] = {0.0, 0.0, 0.0};
        for (uint64_t i = first + t; i < last; i += kBlock) {
            const double gt = depth_load(a.gt, base + i, gt64), pr = depth_load(a.pred, base + i, pr64);
            if (gt > 0.0 && pr > 0.0 && gt < 5.0 && pr < 5.0) {  // a NaN fails
                v[0] = v[0] + 1.0;
                v[1] = v[1] + gt;
                v[2] = v[2] + pr;
            }
        }
        tree_fold<kP1>(v, buf);
        if (t < kP1) p1[((size_t)f * G + g) * kP1 + t] = buf[t][0];
    } else {
        if (t == 0) {
            double n = 0.0, sg = 0.0, sp = 0.0;
            for (uint32_t k = 0; k < G; ++k) {
                const double* s = p1 + ((size_t)f * G + k) * kP1;
                n = n + s[0];
                sg = sg + s[1];
                sp = sp + s[2];
            }
            scale_s = a.with_scale ? (sg / n) / (sp / n) : 1.0;
        }
        __syncthreads();
        const double scale = scale_s;
        double v[kP2] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (uint64_t i = first + t; i < last; i += kBlock) {
            const double gt = depth_load(a.gt, base + i, gt64), pr = depth_load(a.pred, base + i, pr64);
            if (gt > 0.0 && pr > 0.0 && gt < 5.0 && pr < 5.0) {
                const double p = a.with_scale ? pr * scale : pr;
                const double diff = fabs(p - gt);
                const double lg = log(p) - log(gt);
                const double ratio = fmax(gt / p, p / gt);
                v[0] = v[0] + diff / p;
                v[1] = v[1] + diff;
                v[2] = v[2] + (diff * diff) / p;
                v[3] = v[3] + diff * diff;
                v[4] = v[4] + lg * lg;
                v[5] = v[5] + (ratio < 1.25 ? 1.0 : 0.0);       // (counts: whole numbers below 2^31, exact in float64)
                v[6] = v[6] + (ratio < 1.5625 ? 1.0 : 0.0);
                v[7] = v[7] + (ratio < 1.953125 ? 1.0 : 0.0);
            }
        }
        tree_fold<kP2>(v, buf);
        if (t < kP2) p2[((size_t)f * G + g) * kP2 + t] = buf[t][0];
    }
}

__global__ void __launch_bounds__(64) k_m2d_depth_fold(const double* __restrict__ p1, const double* __restrict__ p2, void* table,
                                                       uint32_t G) {
    const uint32_t f = blockIdx.x, t = threadIdx.x;
    if (t >= NVO_M2D_DEPTH_WORDS) return;
    double s = 0.0;
    if (t == 5) {
        for (uint32_t k = 0; k < G; ++k) s = s + p1[((size_t)f * G + k) * kP1];
    } else {
        const uint32_t col = t < 5 ? t : t - 1;  // words 6..8: columns 5..7 of pass 2
        for (uint32_t k = 0; k < G; ++k) s = s + p2[((size_t)f * G + k) * kP2 + col];
    }
    if (t < 5)
        ((double*)table)[(size_t)f * NVO_M2D_DEPTH_WORDS + t] = s;
    else
        ((long long*)table)[(size_t)f * NVO_M2D_DEPTH_WORDS + t] = (long long)s;
}

uint64_t color_tiles(uint32_t H, uint32_t W, uint32_t* tiles_x) {
    const uint64_t tx = ((uint64_t)W + kTW - 1) / kTW, ty = ((uint64_t)H + kTH - 1) / kTH;
    if (tiles_x) *tiles_x = (uint32_t)tx;
    return tx * ty;
}

bool color_shape_ok(uint32_t F, uint32_t H, uint32_t W) {
    return F >= 1 && H >= 1 && W >= 1 && 3ull * F <= 65535ull && (uint64_t)H * W * 3ull < (1ull << 30) &&
           color_tiles(H, W, nullptr) * 3ull * F <= (1ull << 24);
}

bool depth_shape_ok(uint32_t F, uint32_t H, uint32_t W) {
    return F >= 1 && H >= 1 && W >= 1 && F <= 65535u && (uint64_t)H * W < (1ull << 31);
}

}  // namespace

extern "C" {

uint64_t nvo_m2d_color_scratch_bytes(uint32_t F, uint32_t H, uint32_t W) {
    if (!color_shape_ok(F, H, W)) return 0;
    return color_tiles(H, W, nullptr) * 3ull * F * NVO_M2D_COLOR_WORDS * sizeof(uint64_t);
}

int nvo_m2d_color(nvo_stream_t stream, const nvo_m2d_color_args* args) {
    NVO_REQUIRE(args != nullptr, "m2d_color: args is NULL");
    const nvo_m2d_color_args a = *args;
    NVO_REQUIRE(a.a && a.b && a.table && a.scratch, "m2d_color: NULL argument");
    NVO_REQUIRE(a.F >= 1 && a.H >= 1 && a.W >= 1, "m2d_color: %u frames of %u x %u: every size must be at least 1", a.F, a.W, a.H);
    NVO_REQUIRE((uint64_t)a.H * a.W * 3ull < (1ull << 30), "m2d_color: frames of %u x %u have 2^30 values or more (the fixed-point SSIM sum)",
                a.W, a.H);
    NVO_REQUIRE(color_shape_ok(a.F, a.H, a.W), "m2d_color: %u frames of %u x %u are more than one launch takes (3 F <= 65535, 3 F tiles <= 2^24)",
                a.F, a.W, a.H);
    NVO_REQUIRE((((uintptr_t)a.scratch | (uintptr_t)a.table) & 7u) == 0u, "m2d_color: table and scratch must be 8-byte aligned");
    NVO_REQUIRE(!a.is_float || (((uintptr_t)a.a | (uintptr_t)a.b) & 3u) == 0u, "m2d_color: float images must be 4-byte aligned");
    uint32_t tiles_x;
    const uint32_t tiles = (uint32_t)color_tiles(a.H, a.W, &tiles_x);
    TapArgs taps;
    for (int t = 0; t < kTaps; ++t) taps.g[t] = a.taps[t];
    unsigned long long* slots = (unsigned long long*)a.scratch;
    NVO_PROF(stream, "m2d_color");
    if (a.is_float)
        NVO_LAUNCH(k_m2d_color<true>, dim3(tiles, 3u * a.F), dim3(kBlock), 0, (hipStream_t)stream, a.a, a.b, slots, a.H, a.W, tiles_x,
                   tiles, taps);
    else
        NVO_LAUNCH(k_m2d_color<false>, dim3(tiles, 3u * a.F), dim3(kBlock), 0, (hipStream_t)stream, a.a, a.b, slots, a.H, a.W, tiles_x,
                   tiles, taps);
    NVO_CHECK_LAUNCH();
    NVO_LAUNCH(k_m2d_color_fold, dim3(3u * a.F), dim3(kBlock), 0, (hipStream_t)stream, slots, (unsigned long long*)a.table, tiles);
    NVO_CHECK_LAUNCH();
    return NVO_OK;
}

uint32_t nvo_m2d_depth_chunks(uint32_t H, uint32_t W) {
    return depth_shape_ok(1, H, W) ? depth_chunks((uint64_t)H * W) : 0;
}

uint64_t nvo_m2d_depth_scratch_bytes(uint32_t F, uint32_t H, uint32_t W) {
    if (!depth_shape_ok(F, H, W)) return 0;
    return (uint64_t)F * depth_chunks((uint64_t)H * W) * (kP1 + kP2) * sizeof(double);
}

int nvo_m2d_depth(nvo_stream_t stream, const nvo_m2d_depth_args* args) {
    NVO_REQUIRE(args != nullptr, "m2d_depth: args is NULL");
    const nvo_m2d_depth_args a = *args;
    NVO_REQUIRE(a.gt && a.pred && a.table && a.scratch, "m2d_depth: NULL argument");
    NVO_REQUIRE(a.F >= 1 && a.H >= 1 && a.W >= 1, "m2d_depth: %u frames of %u x %u: every size must be at least 1", a.F, a.W, a.H);
    NVO_REQUIRE(depth_shape_ok(a.F, a.H, a.W), "m2d_depth: %u frames of %u x %u: at most 65535 frames of fewer than 2^31 pixels", a.F, a.W,
                a.H);
    NVO_REQUIRE((((uintptr_t)a.scratch | (uintptr_t)a.table) & 7u) == 0u, "m2d_depth: table and scratch must be 8-byte aligned");
    NVO_REQUIRE(((uintptr_t)a.gt & (a.gt_f64 ? 7u : 3u)) == 0u && ((uintptr_t)a.pred & (a.pred_f64 ? 7u : 3u)) == 0u,
                "m2d_depth: misaligned depth images");
    const uint64_t n_pix = (uint64_t)a.H * a.W;
    const uint32_t G = depth_chunks(n_pix);
    const uint32_t chunk = (uint32_t)((n_pix + G - 1) / G);  // G * chunk >= n_pix
    double* p1 = (double*)a.scratch;
    double* p2 = p1 + (size_t)a.F * G * kP1;
    NVO_PROF(stream, "m2d_depth");
    NVO_LAUNCH(k_m2d_depth<1>, dim3(G, a.F), dim3(kBlock), 0, (hipStream_t)stream, a, p1, p2, G, chunk);
    NVO_CHECK_LAUNCH();
    NVO_LAUNCH(k_m2d_depth<2>, dim3(G, a.F), dim3(kBlock), 0, (hipStream_t)stream, a, p1, p2, G, chunk);
    NVO_CHECK_LAUNCH();
    NVO_LAUNCH(k_m2d_depth_fold, dim3(a.F), dim3(64), 0, (hipStream_t)stream, p1, p2, a.table, G);
    NVO_CHECK_LAUNCH();
    return NVO_OK;
}

}  // extern "C"
