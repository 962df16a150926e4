// LPIPS v0.1 (AlexNet features, linear head) of batches of frame pairs (include/nerfvo_hip.h
// section O).  Kernels:
//
//   k_lpips_conv<KS, STRIDE, INGEST>   convolution + bias + ReLU as an implicit GEMM on the exact-fp32 matrix instruction
//                        (v_mfma_f32_32x32x2_f32: fp32 operands, fp32 accumulate, a k-ordered fma chain).  M = output
//                        channels, N = F * Ho * Wo output pixels, K = Cin * KS * KS, padded with zero weights to a multiple
//                        of kBK.  A workgroup of four waves owns a 64 (M) x 128 (N) tile, a wave 32 x 64 of it (two 32 x 32
//                        accumulators).  Per step of kBK: the weights' [kBK][64] slab (pre-packed k-major, so the copy is
//                        contiguous) and the patch's [kBK][128] slab (gathered on the fly: a thread owns ONE output pixel
//                        and walks k) go to LDS, then kBK / 2 instructions per accumulator.  A padded tap, a column past N
//                        and a k past K stage 0.  Every output is the chain over k ascending whatever the batch, so a
//                        frame's values do not depend on what shares the launch.  INGEST 0: the input as it is; 1: the
//                        scaling layer (x - shift[c]) / scale[c] on a float image; 2: a uint8 [F][H][W][3] image,
//                        ((u / 255) * 2 - 1) * 2 - 1 and then the scaling layer, one rounding per operation.
//   k_lpips_pool         max-pool 3 x 3, stride 2, no padding: one thread per output.
//   k_lpips_head         lanes along the pixels of one frame, loops over the channels: the two norms, then
//                        d = sum_c lin[c] * (a_c / n0 - b_c / n1)^2 in fp32, c ascending.  The 256 values of a workgroup fold
//                        as a binary tree in float64; k_lpips_head_fold adds the workgroups' sums in ascending order and
//                        divides by the pixel count.  No atomics.
//
// Bounds: the launchers check pointers, sizes and the products that index; every input tap is compared against H and W,
// every output column against N, every pixel against Ho * Wo before it is touched.
#include "nvo_kernels.h"
#include "../../include/nerfvo_hip.h"

#include <math.h>

namespace {

constexpr int kBM = NVO_LPIPS_TILE_M, kBN = NVO_LPIPS_TILE_N, kBK = NVO_LPIPS_TILE_K, kThreads = 256;
constexpr int kHeadBlock = NVO_LPIPS_HEAD_BLOCK;
static_assert(kBM == 64 && kBN == 128 && kThreads == 256, "four waves, 2 x 2, 32 x 64 each");
static_assert(kBK % 2 == 0 && (kBK * kBM) % kThreads == 0 && (kBK * kBN) % kThreads == 0, "staging loops");
static_assert(kHeadBlock == 256, "tree fold");

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct ConvP {
    const void* x;
    const float* w;     // [Kpad][Cout]
    const float* bias;  // [Cout]
    float* out;         // [F][Cout][Ho][Wo]
    uint32_t Cin, H, W, Cout, Ho, Wo, pad, K, Kpad, N;
    float shift[3], scale[3];
};

template <int KS, int STRIDE, int INGEST>
__global__ void __launch_bounds__(kThreads) k_lpips_conv(const ConvP p) {
    __shared__ float Ws[kBK][kBM];
    __shared__ float Ps[kBK][kBN];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, wm = wave & 1u, wn = wave >> 1;
    const uint32_t m0 = blockIdx.y * kBM, HoWo = p.Ho * p.Wo;

    // the output pixel whose patch this thread gathers
    const uint32_t nl = tid & (kBN - 1), kh = tid / kBN;  // kh: 0 or 1
    const uint32_t n = blockIdx.x * kBN + nl;
    const bool n_ok = n < p.N;
    uint32_t f = 0;
    int iy0 = 0, ix0 = 0;
    if (n_ok) {
        f = n / HoWo;
        const uint32_t pix = n % HoWo, oy = pix / p.Wo, ox = pix % p.Wo;
        iy0 = (int)(oy * STRIDE) - (int)p.pad;
        ix0 = (int)(ox * STRIDE) - (int)p.pad;
    }

    f32x16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = 0.f;

    for (uint32_t k0 = 0; k0 < p.Kpad; k0 += kBK) {
#pragma unroll
        for (int i = 0; i < kBK * kBM / kThreads; ++i) {
            const uint32_t idx = tid + (uint32_t)i * kThreads, kk = idx / kBM, m = idx % kBM;
            Ws[kk][m] = p.w[(size_t)(k0 + kk) * p.Cout + m0 + m];  // k0 + kk < Kpad, m0 + m < Cout
        }
#pragma unroll
        for (int i = 0; i < kBK * kBN / kThreads; ++i) {
            const uint32_t kk = kh + 2u * (uint32_t)i, k = k0 + kk;
            float v = 0.f;
            if (n_ok && k < p.K) {
                const uint32_t ci = k / (KS * KS), r = k % (KS * KS);
                const int iy = iy0 + (int)(r / KS), ix = ix0 + (int)(r % KS);
                if (iy >= 0 && iy < (int)p.H && ix >= 0 && ix < (int)p.W) {
                    if (INGEST == 2) {
                        const uint8_t u = ((const uint8_t*)p.x)[(((size_t)f * p.H + (uint32_t)iy) * p.W + (uint32_t)ix) * 3u + ci];
                        v = (((float)u / 255.0f) * 2.0f - 1.0f) * 2.0f - 1.0f;
                    } else {
                        v = ((const float*)p.x)[(((size_t)f * p.Cin + ci) * p.H + (uint32_t)iy) * p.W + (uint32_t)ix];
                    }
                    if (INGEST != 0) {  // Cin == 3 (the launcher checks)
                        const float sh = ci == 0 ? p.shift[0] : (ci == 1 ? p.shift[1] : p.shift[2]);
                        const float sc = ci == 0 ? p.scale[0] : (ci == 1 ? p.scale[1] : p.scale[2]);
                        v = (v - sh) / sc;
                    }
                }
            }
            Ps[kk][nl] = v;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < kBK; kk += 2) {
            const uint32_t kr = (uint32_t)kk + (lane >> 5), c = lane & 31u;
            const float a = Ws[kr][wm * 32u + c];
            const float b0 = Ps[kr][wn * 64u + c], b1 = Ps[kr][wn * 64u + 32u + c];
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b0, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1, acc1, 0, 0, 0);
        }
        __syncthreads();
    }

    // C/D map: column = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const uint32_t col = blockIdx.x * kBN + wn * 64u + (uint32_t)j * 32u + (lane & 31u);
        if (col >= p.N) continue;
        const uint32_t fo = col / HoWo, pix = col % HoWo;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const uint32_t m = m0 + wm * 32u + (uint32_t)((r & 3) + 8 * (r >> 2)) + 4u * (lane >> 5);
            const float v = (j == 0 ? acc0[r] : acc1[r]) + p.bias[m];
            p.out[((size_t)fo * p.Cout + m) * HoWo + pix] = v > 0.f ? v : 0.f;
        }
    }
}

__global__ void __launch_bounds__(256) k_lpips_pool(const float* __restrict__ x, float* __restrict__ out, uint64_t total, uint32_t H,
                                                    uint32_t W, uint32_t Ho, uint32_t Wo) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= total) return;
    const uint32_t ox = (uint32_t)(i % Wo), oy = (uint32_t)((i / Wo) % Ho);
    const uint64_t fc = i / ((uint64_t)Wo * Ho);
    const float* src = x + (fc * H + 2u * oy) * W + 2u * ox;  // rows 2 oy .. 2 oy + 2 < H, columns 2 ox .. 2 ox + 2 < W
    float m = -INFINITY;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const float v = src[(size_t)dy * W + dx];
            if (v > m || v != v) m = v;
        }
    out[i] = m;
}

__global__ void __launch_bounds__(kHeadBlock) k_lpips_head(const float* __restrict__ f0, const float* __restrict__ f1,
                                                           const float* __restrict__ lin, float* __restrict__ map,
                                                           double* __restrict__ partial, uint32_t C, uint32_t HW, uint32_t G) {
    __shared__ double buf[kHeadBlock];
    const uint32_t g = blockIdx.x, f = blockIdx.y, t = threadIdx.x, px = g * kHeadBlock + t;
    double d = 0.0;
    if (px < HW) {
        const float* a = f0 + (size_t)f * C * HW + px;
        const float* b = f1 + (size_t)f * C * HW + px;
        float s0 = 0.f, s1 = 0.f;
        for (uint32_t c = 0; c < C; ++c) {
            const float u = a[(size_t)c * HW], v = b[(size_t)c * HW];
            s0 = s0 + u * u;
            s1 = s1 + v * v;
        }
        const float n0 = sqrtf(s0) + 1e-10f, n1 = sqrtf(s1) + 1e-10f;
        float acc = 0.f;
        for (uint32_t c = 0; c < C; ++c) {
            const float e = a[(size_t)c * HW] / n0 - b[(size_t)c * HW] / n1;
            acc = acc + lin[c] * (e * e);
        }
        if (map) map[(size_t)f * HW + px] = acc;
        d = (double)acc;
    }
    buf[t] = d;
    __syncthreads();
    for (uint32_t s = kHeadBlock / 2; s >= 1; s >>= 1) {
        if (t < s) buf[t] = buf[t] + buf[t + s];
        __syncthreads();
    }
    if (t == 0) partial[(size_t)f * G + g] = buf[0];
}

__global__ void __launch_bounds__(64) k_lpips_head_fold(const double* __restrict__ partial, float* __restrict__ out, uint32_t F,
                                                        uint32_t G, uint32_t HW, int accumulate) {
    const uint32_t f = blockIdx.x * 64u + threadIdx.x;
    if (f >= F) return;
    double s = 0.0;
    for (uint32_t g = 0; g < G; ++g) s = s + partial[(size_t)f * G + g];
    const float v = (float)(s / (double)HW);
    out[f] = accumulate ? out[f] + v : v;
}

bool conv_out(uint32_t in, uint32_t ks, uint32_t stride, uint32_t pad, uint32_t* out) {
    if ((uint64_t)in + 2ull * pad < ks) return false;
    *out = (uint32_t)(((uint64_t)in + 2ull * pad - ks) / stride + 1u);
    return true;
}

bool head_shape_ok(uint32_t F, uint32_t C, uint32_t HW) {
    return F >= 1 && C >= 1 && HW >= 1 && F <= 65535u && (uint64_t)F * C * HW < (1ull << 40);
}

template <int KS, int STRIDE, int INGEST>
int launch_conv(hipStream_t stream, const ConvP& p, dim3 grid) {
    NVO_LAUNCH((k_lpips_conv<KS, STRIDE, INGEST>), grid, dim3(kThreads), 0, stream, p);
    NVO_CHECK_LAUNCH();
    return NVO_OK;
}

}  // namespace

extern "C" {

uint32_t nvo_lpips_conv_kpad(uint32_t K) {
    return K >= 1 && K <= (1u << 24) ? (uint32_t)nvo_round_up(K, kBK) : 0;
}

int nvo_lpips_conv(nvo_stream_t stream, const nvo_lpips_conv_args* args) {
    NVO_REQUIRE(args != nullptr, "lpips_conv: args is NULL");
    const nvo_lpips_conv_args a = *args;
    NVO_REQUIRE(a.x && a.weights && a.bias && a.out, "lpips_conv: NULL argument");
    NVO_REQUIRE(a.F >= 1 && a.Cin >= 1 && a.H >= 1 && a.W >= 1, "lpips_conv: %u images of %u x %u x %u: every size must be at least 1", a.F,
                a.Cin, a.W, a.H);
    NVO_REQUIRE((a.ksize == 11 && a.stride == 4) || (a.ksize == 5 && a.stride == 1) || (a.ksize == 3 && a.stride == 1),
                "lpips_conv: kernel %u stride %u has no instance (AlexNet's three: 11/4, 5/1, 3/1)", a.ksize, a.stride);
    NVO_REQUIRE(a.pad < a.ksize, "lpips_conv: padding %u of a %u-tap kernel", a.pad, a.ksize);
    NVO_REQUIRE(a.Cout >= kBM && a.Cout % kBM == 0 && a.Cout <= 65535u * kBM, "lpips_conv: %u output channels: a multiple of %d", a.Cout, kBM);
    NVO_REQUIRE(a.ingest >= 0 && a.ingest <= 2 && (a.ingest == 0 || (a.Cin == 3 && a.ksize == 11)),
                "lpips_conv: ingest %d with %u channels and kernel %u (the scaling layer feeds conv1: 3 channels, 11 taps)", a.ingest, a.Cin, a.ksize);
    uint32_t Ho, Wo;
    NVO_REQUIRE(conv_out(a.H, a.ksize, a.stride, a.pad, &Ho) && conv_out(a.W, a.ksize, a.stride, a.pad, &Wo),
                "lpips_conv: a %u x %u image is smaller than the %u-tap kernel with padding %u", a.W, a.H, a.ksize, a.pad);
    const uint64_t K = (uint64_t)a.Cin * a.ksize * a.ksize, N = (uint64_t)a.F * Ho * Wo;
    NVO_REQUIRE(K <= (1u << 24) && a.Kpad == nvo_lpips_conv_kpad((uint32_t)K), "lpips_conv: Kpad %u is not nvo_lpips_conv_kpad(%llu)", a.Kpad,
                (unsigned long long)K);
    NVO_REQUIRE(N < (1ull << 31) && (uint64_t)a.F * a.Cin * a.H * a.W < (1ull << 40) && N * a.Cout < (1ull << 40),
                "lpips_conv: %u images of %u x %u: more output pixels than one launch takes (F Ho Wo < 2^31)", a.F, a.W, a.H);
    NVO_REQUIRE((((uintptr_t)a.weights | (uintptr_t)a.bias | (uintptr_t)a.out) & 3u) == 0u && (a.ingest == 2 || ((uintptr_t)a.x & 3u) == 0u),
                "lpips_conv: float arrays must be 4-byte aligned");
    ConvP p;
    p.x = a.x;
    p.w = a.weights;
    p.bias = a.bias;
    p.out = a.out;
    p.Cin = a.Cin, p.H = a.H, p.W = a.W, p.Cout = a.Cout, p.Ho = Ho, p.Wo = Wo, p.pad = a.pad;
    p.K = (uint32_t)K, p.Kpad = a.Kpad, p.N = (uint32_t)N;
    for (int c = 0; c < 3; ++c) p.shift[c] = a.shift[c], p.scale[c] = a.scale[c];
    const dim3 grid(nvo_div_up(N, kBN), a.Cout / kBM);
    NVO_PROF(stream, "lpips_conv_k%u_c%u", a.ksize, a.Cin);
    if (a.ksize == 11 && a.ingest == 2) return launch_conv<11, 4, 2>((hipStream_t)stream, p, grid);
    if (a.ksize == 11 && a.ingest == 1) return launch_conv<11, 4, 1>((hipStream_t)stream, p, grid);
    if (a.ksize == 11) return launch_conv<11, 4, 0>((hipStream_t)stream, p, grid);
    if (a.ksize == 5) return launch_conv<5, 1, 0>((hipStream_t)stream, p, grid);
    return launch_conv<3, 1, 0>((hipStream_t)stream, p, grid);
}

int nvo_lpips_pool(nvo_stream_t stream, const nvo_lpips_pool_args* args) {
    NVO_REQUIRE(args != nullptr, "lpips_pool: args is NULL");
    const nvo_lpips_pool_args a = *args;
    NVO_REQUIRE(a.x && a.out, "lpips_pool: NULL argument");
    NVO_REQUIRE(a.planes >= 1 && a.H >= 3 && a.W >= 3, "lpips_pool: %u planes of %u x %u: a 3 x 3 window needs 3 x 3", a.planes, a.W, a.H);
    const uint32_t Ho = (a.H - 3u) / 2u + 1u, Wo = (a.W - 3u) / 2u + 1u;
    const uint64_t total = (uint64_t)a.planes * Ho * Wo;
    NVO_REQUIRE((uint64_t)a.planes * a.H * a.W < (1ull << 40) && total < (1ull << 39), "lpips_pool: %u planes of %u x %u are more than one launch takes",
                a.planes, a.W, a.H);
    NVO_REQUIRE((((uintptr_t)a.x | (uintptr_t)a.out) & 3u) == 0u, "lpips_pool: float arrays must be 4-byte aligned");
    NVO_PROF(stream, "lpips_pool");
    NVO_LAUNCH(k_lpips_pool, dim3(nvo_div_up(total, 256)), dim3(256), 0, (hipStream_t)stream, a.x, a.out, total, a.H, a.W, Ho, Wo);
    NVO_CHECK_LAUNCH();
    return NVO_OK;
}

uint64_t nvo_lpips_head_scratch_bytes(uint32_t F, uint32_t C, uint32_t HW) {
    if (!head_shape_ok(F, C, HW)) return 0;
    return (uint64_t)F * nvo_div_up(HW, kHeadBlock) * sizeof(double);
}

int nvo_lpips_head(nvo_stream_t stream, const nvo_lpips_head_args* args) {
    NVO_REQUIRE(args != nullptr, "lpips_head: args is NULL");
    const nvo_lpips_head_args a = *args;
    NVO_REQUIRE(a.f0 && a.f1 && a.lin && a.scratch && a.out, "lpips_head: NULL argument (map alone may be NULL)");
    NVO_REQUIRE(head_shape_ok(a.F, a.C, a.HW), "lpips_head: %u maps of %u channels x %u pixels: 1 <= F <= 65535, F C HW < 2^40", a.F, a.C, a.HW);
    NVO_REQUIRE(((uintptr_t)a.scratch & 7u) == 0u, "lpips_head: scratch must be 8-byte aligned");
    NVO_REQUIRE((((uintptr_t)a.f0 | (uintptr_t)a.f1 | (uintptr_t)a.lin | (uintptr_t)a.map | (uintptr_t)a.out) & 3u) == 0u,
                "lpips_head: float arrays must be 4-byte aligned");
    const uint32_t G = nvo_div_up(a.HW, kHeadBlock);
    NVO_PROF(stream, "lpips_head_c%u", a.C);
    NVO_LAUNCH(k_lpips_head, dim3(G, a.F), dim3(kHeadBlock), 0, (hipStream_t)stream, a.f0, a.f1, a.lin, a.map, (double*)a.scratch, a.C, a.HW, G);
    NVO_CHECK_LAUNCH();
    NVO_LAUNCH(k_lpips_head_fold, dim3(nvo_div_up(a.F, 64)), dim3(64), 0, (hipStream_t)stream, (const double*)a.scratch, a.out, a.F, G, a.HW,
               a.accumulate);
    NVO_CHECK_LAUNCH();
    return NVO_OK;
}

}  // extern "C"
