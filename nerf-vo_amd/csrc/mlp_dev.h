// Device-side building blocks of the fully fused MLP that other kernels share with mlp_impl.h: the matrix-core
// wrappers, the activation + pack step, the A-operand weight fragments with their LDS staging, and one layer's
// product.  The small-grid forward of grid.hip runs the proposal density network (10 -> 16 -> 1) as its epilogue
// through exactly these functions, so that it produces the bits k_mlp_fwd produces.
//
// Compiled once per 16-bit element type, like mlp_impl.h: define NVO_MLP_BF16 (0 | 1) before including.  The text lands
// in namespace nvo_mlp_dev_f16 (T = _Float16, v_mfma_f32_16x16x16_f16) or nvo_mlp_dev_bf16 (T = __bf16,
// v_mfma_f32_16x16x16_bf16); a translation unit that needs both includes the file twice (no include guard).
#include "nvo_kernels.h"

#ifndef NVO_MLP_BF16
#error "define NVO_MLP_BF16 (0 | 1) before including mlp_dev.h"
#endif

namespace {
#if NVO_MLP_BF16
namespace nvo_mlp_dev_bf16 {
typedef __bf16 T;
#else
namespace nvo_mlp_dev_f16 {
typedef _Float16 T;
#endif
typedef T T4 __attribute__((ext_vector_type(4)));
typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int kMlpBlock = 256;  // threads of the MLP kernels' workgroups (RowStage strides by it; any block >= it works)

// one MFMA 16x16x16 (K = 16: 4 operand elements per lane); fp16 and bf16 share the register layout
__device__ __forceinline__ f4 mfma16(T4 a, T4 b, f4 c) {
#if NVO_MLP_BF16
    typedef short s4 __attribute__((ext_vector_type(4)));
    s4 as, bs;
    __builtin_memcpy(&as, &a, sizeof(as));
    __builtin_memcpy(&bs, &b, sizeof(bs));
    return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(as, bs, c, 0, 0, 0);
#else
    return __builtin_amdgcn_mfma_f32_16x16x16f16(a, b, c, 0, 0, 0);
#endif
}

// gfx950's K = 32 form, operands given as two K = 16 fragments each: element j < 4 of lane group g pairs feature
// 16 (2t) + 4g + j of both operands, j >= 4 feature 16 (2t + 1) + 4g + (j - 4) -- the same 32 products as two chained
// 16x16x16 instructions in HALF the matrix-core time (the K = 16 form runs at the MI300 rate on this chip); the order of
// the fp32 additions inside differs, which forward and recomputing backward share.
#ifdef NVO_MLP_K16  // (A/B builds: NVO_EXTRA_CXXFLAGS=-DNVO_MLP_K16)
constexpr bool kUseK32 = false;
#else
constexpr bool kUseK32 = true;
#endif
__device__ __forceinline__ f4 mfma32(T4 a_lo, T4 a_hi, T4 b_lo, T4 b_hi, f4 c) {
    typedef T T8 __attribute__((ext_vector_type(8)));
    const T8 a = __builtin_shufflevector(a_lo, a_hi, 0, 1, 2, 3, 4, 5, 6, 7);
    const T8 b = __builtin_shufflevector(b_lo, b_hi, 0, 1, 2, 3, 4, 5, 6, 7);
#if NVO_MLP_BF16
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
#else
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
#endif
}

__device__ __forceinline__ float act_fwd(int act, float v) {
    if (act == NVO_ACT_RELU) return fmaxf(v, 0.f);
    if (act == NVO_ACT_SIGMOID) return 1.f / (1.f + __expf(-v));
    return v;
}

__device__ __forceinline__ T4 pack_act(int act, f4 v) {
    T4 r;
    r[0] = (T)act_fwd(act, v[0]);
    r[1] = (T)act_fwd(act, v[1]);
    r[2] = (T)act_fwd(act, v[2]);
    r[3] = (T)act_fwd(act, v[3]);
    return r;
}

// A-operand fragments of W[N_OUT][K_IN] (row-major): f[tn][tk] = W[16tn + (l&15)][16tk + 4g + j]
template <int N_OUT, int K_IN>
struct WFrag {
    T4 f[N_OUT / 16][K_IN / 16];
    __device__ __forceinline__ void load(const T* __restrict__ W, int lane) {
        const int r = lane & 15, g = lane >> 4;
#pragma unroll
        for (int tn = 0; tn < N_OUT / 16; ++tn)
#pragma unroll
            for (int tk = 0; tk < K_IN / 16; ++tk)
                f[tn][tk] = *reinterpret_cast<const T4*>(W + (size_t)(16 * tn + r) * K_IN + 16 * tk + 4 * g);
    }
    // the same fragments from the workgroup's row-major LDS copy of W (row stride K_IN + 4 halfs, see RowStage): the
    // direct form touches 16 rows x 32 bytes per load instruction -- 16 cache lines for 512 bytes -- and every wave of
    // the grid pays it for the whole weight set
    __device__ __forceinline__ void load_staged(const T* stage, int lane) {
        const int r = lane & 15, g = lane >> 4;
#pragma unroll
        for (int tn = 0; tn < N_OUT / 16; ++tn)
#pragma unroll
            for (int tk = 0; tk < K_IN / 16; ++tk)
                f[tn][tk] = *reinterpret_cast<const T4*>(stage + (16 * tn + r) * (K_IN + 4) + 16 * tk + 4 * g);
    }
};

// One matrix on its way global -> registers -> LDS staging (row stride K_IN + 4 halfs).  Split in two so that a kernel
// can have the loads of ALL its matrices in flight before the first LDS store waits for one of them.
template <int N_OUT, int K_IN>
struct RowStage {
    static constexpr int kT4 = N_OUT * K_IN / 4, kTrips = (kT4 + kMlpBlock - 1) / kMlpBlock, kHalfs = N_OUT * (K_IN + 4);
    T4 v[kTrips];
    __device__ __forceinline__ void issue(const T* __restrict__ W) {
#pragma unroll
        for (int i = 0; i < kTrips; ++i) {
            const int e = (int)threadIdx.x + i * kMlpBlock;
            v[i] = *reinterpret_cast<const T4*>(W + 4 * (size_t)(e < kT4 ? e : 0));
        }
    }
    __device__ __forceinline__ void store(T* stage) const {
#pragma unroll
        for (int i = 0; i < kTrips; ++i) {
            const int e = (int)threadIdx.x + i * kMlpBlock;
            if (e < kT4) *reinterpret_cast<T4*>(stage + ((4 * e) / K_IN) * (K_IN + 4) + (4 * e) % K_IN) = v[i];
        }
    }
};

// H_out^T tile = W * H_in^T
template <int N_OUT, int K_IN>
__device__ __forceinline__ void layer_mm(const WFrag<N_OUT, K_IN>& w, const T4 (&in)[K_IN / 16],
                                         f4 (&acc)[N_OUT / 16]) {
#pragma unroll
    for (int tn = 0; tn < N_OUT / 16; ++tn) {
        f4 c = {0.f, 0.f, 0.f, 0.f};
        if constexpr ((K_IN / 16) % 2 == 0 && kUseK32) {
#pragma unroll
            for (int tk = 0; tk < K_IN / 16; tk += 2) c = mfma32(w.f[tn][tk], w.f[tn][tk + 1], in[tk], in[tk + 1], c);
        } else {
#pragma unroll
            for (int tk = 0; tk < K_IN / 16; ++tk) c = mfma16(w.f[tn][tk], in[tk], c);
        }
        acc[tn] = c;
    }
}

}  // namespace nvo_mlp_dev_{f16,bf16}
}  // namespace
