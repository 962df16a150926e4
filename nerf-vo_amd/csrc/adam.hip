// Fused Adam step over a flat fp32 parameter range for gfx950: reads grad / m / v / master weight,
// writes m / v / master weight and the fp16 working copy the kernels consume, in one pass
// (28 B + 2 B per parameter -- the HBM floor of the optimiser).
// Semantics = torch.optim.Adam (no AMSGrad, L2 weight decay folded into the gradient) as the
// reference configures it: AdamOptimizerConfig(lr=1e-2|1e-4, eps=1e-15)
// (/root/reference/nerf_vo/mapping/nerfstudio.py:84-100); the GradScaler "skip the step when a
// non-finite gradient was found" behaviour (mixed_precision=True, nerfstudio.py:59) is the
// optional skip flag.  CPU restatement: oracle/nerfacto.py::adam_reference.
#include "nvo_kernels.h"
#include "../../include/nerfvo_hip.h"

#include <string.h>

namespace {

__device__ __forceinline__ float load_grad(const float* g, uint64_t i) { return g[i]; }
__device__ __forceinline__ float load_grad(const _Float16* g, uint64_t i) { return (float)g[i]; }
// bfloat16 = the upper half of an fp32: same exponent range, 8 significant bits.  The compressed gradient exchange
// uses it rather than fp16 because Adam (eps 1e-15) turns ANY non-zero gradient into a full-size step, so the
// tiny gradients of rarely hit hash-grid entries must not flush to zero (fp16 underflows below 6e-8).
struct Bf16 { uint16_t bits; };
__device__ __forceinline__ float load_grad(const Bf16* g, uint64_t i) { return __uint_as_float((uint32_t)g[i].bits << 16); }
__device__ __forceinline__ uint16_t to_bf16(float x) {
    const uint32_t u = __float_as_uint(x);
    if ((u & 0x7F800000u) == 0x7F800000u) return (uint16_t)((u >> 16) | ((u & 0xFFFFu) ? 0x40u : 0u));  // inf / NaN stay so
    return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);  // round to nearest even
}

typedef NvoAdamHyper AdamHyper;  // (nvo_common.h: shared with the hash-grid backward's fused step)

// Format of the 16-bit working copy the kernels read: fp16 everywhere except inside up to 4 element ranges
// [lo, hi) of the flat buffer, which are bfloat16 (bf16 MLP mode: the fused-MLP weights and the appearance
// embedding; the hash tables stay fp16 -- 11 significant bits for entries that are interpolated in fp32).
// Range bounds are multiples of 4 (checked on the host), so a 4-element vector never straddles a boundary.
constexpr uint32_t kMaxBf16Ranges = 4;
struct Copy16Fmt {
    uint32_t n;
    uint64_t lo[kMaxBf16Ranges], hi[kMaxBf16Ranges];
    __device__ __forceinline__ bool is_bf16(uint64_t i) const {
        bool r = false;
#pragma unroll
        for (uint32_t k = 0; k < kMaxBf16Ranges; ++k) r = r || (k < n && i >= lo[k] && i < hi[k]);
        return r;
    }
};

__device__ __forceinline__ void adam_one(float& p, float& m, float& v, float g, const AdamHyper& h) {
    nvo_adam_one(p, m, v, g, h);
}

// GT = float (local gradient), _Float16 or Bf16 (the 2-byte buffer a compressed all-reduce leaves behind).
// The body works on 4 consecutive parameters per thread through 16-byte accesses when the range is
// 16-byte aligned (HBM-bound kernel: 28 B + 2 B per parameter), scalar otherwise / for the tail.
// base: index of p[0] in the flat buffer (what Copy16Fmt's ranges refer to)
// Optional weight average of the stepped elements (tcnn EmaOptimizer; k_ema_update's arithmetic on the value just
// written, term for term): ema / ema16 start at the range like p does; the 16-byte form needs them aligned like p / p16.
struct AdamEma {
    float* ema;
    nvo_h16* ema16;
    float keep, take, inv_debias;
};
template <typename GT>
__device__ __forceinline__ void adam_range(uint64_t n, float* __restrict__ p, nvo_h16* __restrict__ p16,
                                           const GT* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                           const AdamHyper& h, int vec4, uint32_t block_id, uint32_t n_blocks,
                                           const Copy16Fmt& fmt, uint64_t base, const AdamEma& ea = AdamEma{}) {
    const uint64_t stride = (uint64_t)n_blocks * blockDim.x;
    const uint64_t tid = (uint64_t)block_id * blockDim.x + threadIdx.x;
    uint64_t done = 0;
    if (vec4) {
        const uint64_t n4 = n >> 2;
        for (uint64_t q = tid; q < n4; q += stride) {
            float4 pv = reinterpret_cast<float4*>(p)[q];
            float4 mv = reinterpret_cast<float4*>(m)[q];
            float4 vv = reinterpret_cast<float4*>(v)[q];
            const uint64_t i = q << 2;
            adam_one(pv.x, mv.x, vv.x, load_grad(g, i + 0), h);
            adam_one(pv.y, mv.y, vv.y, load_grad(g, i + 1), h);
            adam_one(pv.z, mv.z, vv.z, load_grad(g, i + 2), h);
            adam_one(pv.w, mv.w, vv.w, load_grad(g, i + 3), h);
            reinterpret_cast<float4*>(p)[q] = pv;
            reinterpret_cast<float4*>(m)[q] = mv;
            reinterpret_cast<float4*>(v)[q] = vv;
            if (p16) {
                const bool bf = fmt.is_bf16(base + i);
                *reinterpret_cast<uint2*>(p16 + i) = make_uint2(nvo_cvt16x2(pv.x, pv.y, bf), nvo_cvt16x2(pv.z, pv.w, bf));
            }
            if (ea.ema) {
                float4 ev = reinterpret_cast<float4*>(ea.ema)[q];
                ev.x = (ev.x * ea.keep + pv.x * ea.take) * ea.inv_debias;
                ev.y = (ev.y * ea.keep + pv.y * ea.take) * ea.inv_debias;
                ev.z = (ev.z * ea.keep + pv.z * ea.take) * ea.inv_debias;
                ev.w = (ev.w * ea.keep + pv.w * ea.take) * ea.inv_debias;
                reinterpret_cast<float4*>(ea.ema)[q] = ev;
                if (ea.ema16)
                    *reinterpret_cast<uint2*>(ea.ema16 + i) =
                        make_uint2(nvo_cvt16x2(ev.x, ev.y, false), nvo_cvt16x2(ev.z, ev.w, false));
            }
        }
        done = n4 << 2;
    }
    for (uint64_t i = done + tid; i < n; i += stride) {
        float pi = p[i], mi = m[i], vi = v[i];
        adam_one(pi, mi, vi, load_grad(g, i), h);
        p[i] = pi;
        m[i] = mi;
        v[i] = vi;
        if (p16) p16[i] = nvo_cvt16(pi, fmt.is_bf16(base + i));
        if (ea.ema) {
            const float e = (ea.ema[i] * ea.keep + pi * ea.take) * ea.inv_debias;
            ea.ema[i] = e;
            if (ea.ema16) ea.ema16[i] = nvo_cvt16(e, false);
        }
    }
}

// Up to 4 parameter groups (own range, learning rate, step count, flag word and weight decay each) of ONE flat buffer
// in one launch: the groups of a training step differ only in those scalars, and a launch per group costs ~8 us of
// dispatch for what may be a thousand parameters (the camera group).  Blocks [first_block[k], first_block[k + 1])
// serve group k.
constexpr uint32_t kAdamMaxGroups = 4;
struct AdamGroups {
    uint32_t n_groups;
    uint32_t first_block[kAdamMaxGroups + 1];
    uint64_t offset[kAdamMaxGroups], n[kAdamMaxGroups];
    float lr[kAdamMaxGroups], bias1[kAdamMaxGroups], bias2_sqrt[kAdamMaxGroups];
    const float* hyper_dev[kAdamMaxGroups];
    const float* bias_dev[kAdamMaxGroups];  // {1 - beta1^t, sqrt(1 - beta2^t)} kept by nvo_opt_commit (nvo_adam_group::bias_dev)
    int vec4[kAdamMaxGroups];
    uint32_t slot[kAdamMaxGroups];  // index of the group's skip flag
    float wd[kAdamMaxGroups];       // L2 weight decay of the group
};

__device__ void opt_commit_thread(uint32_t n_groups, uint32_t active_mask, uint32_t scale_mask, uint32_t* __restrict__ applied,
                                  const uint32_t* __restrict__ skip_flags, float* __restrict__ scale,
                                  uint32_t* __restrict__ growth_tracker, float growth, float backoff, uint32_t interval,
                                  float min_scale, float max_scale, float* __restrict__ bias, float beta1, float beta2);

template <typename GT>
__global__ void __launch_bounds__(256)
k_adam_groups(AdamGroups gr, float* __restrict__ p, nvo_h16* __restrict__ p16, const GT* __restrict__ g,
              float* __restrict__ m, float* __restrict__ v, AdamHyper h, const uint32_t* __restrict__ skip_flags,
              Copy16Fmt fmt, const float* __restrict__ loss_scale_dev, nvo_adam_tail t) {
    uint32_t k = 0;
    while (k + 1 < gr.n_groups && blockIdx.x >= gr.first_block[k + 1]) ++k;
    __shared__ float fac[2];
    if (t.ema) {  // (uniform) the factors of k_ema_update, from the counter as it stands
        if (threadIdx.x == 0) {
            const double d = (double)t.ema_decay, st = (double)(*t.ema_step_dev) + 1.0;
            fac[0] = (float)(d * (1.0 - pow(d, st - 1.0)));
            fac[1] = (float)(1.0 / (1.0 - pow(d, st)));
        }
        __syncthreads();
    }
    // GradScaler.step decides per optimiser: a group is skipped iff ITS gradients held a non-finite value
    if (!(skip_flags && skip_flags[gr.slot[k]])) {
        h.lr = gr.lr[k];
        h.bias1 = gr.bias1[k];
        h.bias2_sqrt = gr.bias2_sqrt[k];
        h.weight_decay = gr.wd[k];
        if (gr.hyper_dev[k]) {
            h.lr = gr.hyper_dev[k][0];
            h.bias1 = gr.hyper_dev[k][1];
            h.bias2_sqrt = gr.hyper_dev[k][2];
        }
        if (gr.bias_dev[k]) {
            // torch.optim.Adam under GradScaler.step: state['step'] counts the APPLIED steps only -- the counter and the
            // bias corrections of the NEXT applied step live on the device; the commit advances them behind this launch
            // (or as its last act: nvo_adam_tail) iff the group was not skipped
            h.bias1 = gr.bias_dev[k][0];
            h.bias2_sqrt = gr.bias_dev[k][1];
        }
        if (loss_scale_dev) h.grad_scale = 1.0f / *loss_scale_dev;  // dynamic loss scale (GradScaler state on the device)
        const uint64_t o = gr.offset[k];
        AdamEma ea{};
        if (t.ema) ea = AdamEma{t.ema + o, t.ema_half ? (nvo_h16*)t.ema_half + o : nullptr, fac[0], 1.0f - t.ema_decay, fac[1]};
        adam_range<GT>(gr.n[k], p + o, p16 ? p16 + o : nullptr, g + o, m + o, v + o, h, gr.vec4[k],
                       blockIdx.x - gr.first_block[k], gr.first_block[k + 1] - gr.first_block[k], fmt, o, ea);
    }
    if (!t.done_counter) return;  // (uniform)
    // Check-in without a round trip: every workgroup adds one to the counter (fire and forget -- a RETURNING atomic per
    // workgroup on one address cost 75 ns each, +90 us on a 1200-workgroup launch), the LAST workgroup of the grid waits
    // for the others and commits (the final load is an acquire).  Workgroups are dispatched in index order, so everything it waits for is resident or
    // done: no deadlock.  What the ordering has to guarantee is only that every READ of the scalars the commit changes
    // (bias corrections, loss scale, learning rates, average counter) precedes it: those loads were consumed before the
    // workgroup's first store, long before its check-in -- so relaxed atomics at agent scope do (they act at the coherent
    // level; a release / __threadfence() per workgroup is an L2 write-back on this multi-XCD part, and nothing here needs
    // another workgroup's WRITES).
    __syncthreads();
    if (blockIdx.x != gridDim.x - 1u) {
        if (threadIdx.x == 0) __hip_atomic_fetch_add(t.done_counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    // The counter must arrive at EXACTLY gridDim.x - 1.  A counter someone left dirty (an aborted launch, a caller that
    // did not zero it) ends above that and a stall ends below: either way the wait runs out (~0.5 s) and the launch raises
    // a STICKY error instead of committing -- bit 31 of the counter, which the host checks wherever it reads the step's
    // results (nvo_adam_tail::done_counter) -- and neither commits nor resets: committing on a dirty counter could run
    // before every workgroup has read the scalars the commit changes, i.e. silent optimiser-state corruption.
    __shared__ uint32_t s_commit;
    if (threadIdx.x == 0) {
        uint32_t ok = 0u;
        for (uint32_t spin = 0; spin < (1u << 20); ++spin) {
            const uint32_t v = __hip_atomic_load(t.done_counter, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
            if (v & 0x80000000u) break;  // (an earlier launch already failed: stay failed)
            if (v == gridDim.x - 1u) {
                ok = 1u;
                break;
            }
            if (v > gridDim.x - 1u) break;  // (dirty: it can only grow)
            __builtin_amdgcn_s_sleep(16);
        }
        if (!ok) __hip_atomic_fetch_or(t.done_counter, 0x80000000u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_commit = ok;
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_commit) {
        const nvo_opt_commit_args& c = t.commit;  // (its skip_flags / betas are the launch's: checked on the host)
        if (c.applied || c.scale)
            opt_commit_thread(c.n_groups, c.active_mask, c.scale_mask, c.applied, skip_flags, c.scale, c.growth_tracker,
                              c.growth_factor, c.backoff_factor, c.growth_interval, c.min_scale, c.max_scale, c.bias, h.beta1,
                              h.beta2);
        if (t.ema_commit && !(skip_flags && skip_flags[t.ema_flag_slot] != 0u)) *t.ema_step_dev += 1u;  // (k_ema_commit)
        *t.done_counter = 0u;  // (the next launch / replay counts from zero again)
    }
}

// A pure streaming read: 16-byte loads, four of them in flight per thread (the scalar grid-stride form ran at
// 2.6 TB/s).  Non-finite <=> exponent field all ones; checked on the raw bits.
template <typename GT>
__device__ __forceinline__ bool nonfinite_range(uint64_t n, const GT* __restrict__ g, uint32_t block_id,
                                                uint32_t n_blocks) {
    constexpr uint32_t kPer = 16 / sizeof(GT);  // elements per 16-byte load
    const uint64_t n_vec = (((uintptr_t)g & 15u) == 0u) ? n / kPer : 0u;
    const uint4* __restrict__ gv = reinterpret_cast<const uint4*>(g);
    const uint64_t stride = (uint64_t)n_blocks * blockDim.x;
    const uint64_t tid = (uint64_t)block_id * blockDim.x + threadIdx.x;
    bool bad = false;
    auto check = [&](uint4 q) {
        if constexpr (sizeof(GT) == 4) {
            bad = bad || (q.x & 0x7F800000u) == 0x7F800000u || (q.y & 0x7F800000u) == 0x7F800000u ||
                  (q.z & 0x7F800000u) == 0x7F800000u || (q.w & 0x7F800000u) == 0x7F800000u;
        } else {
            constexpr uint32_t lo = sizeof(GT) == 2 && __is_same(GT, Bf16) ? 0x7F80u : 0x7C00u;  // exponent field
            const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int k = 0; k < 4; ++k)
                bad = bad || (w[k] & lo) == lo || (w[k] & (lo << 16)) == (lo << 16);
        }
    };
    uint64_t i = tid;
    for (; i + 3 * stride < n_vec; i += 4 * stride) {
        const uint4 a = gv[i], b = gv[i + stride], c = gv[i + 2 * stride], d = gv[i + 3 * stride];
        check(a);
        check(b);
        check(c);
        check(d);
    }
    for (; i < n_vec; i += stride) check(gv[i]);
    for (uint64_t j = n_vec * kPer + tid; j < n; j += stride) {  // unaligned base or tail
        const float x = load_grad(g, j);
        bad = bad || !(fabsf(x) <= 3.0e38f);
    }
    return bad;
}

// Up to 8 spans of one gradient buffer in one launch, each with the flag word it raises (several spans may raise the
// same word).  Blocks [first_block[k], first_block[k + 1]) serve span k.
constexpr uint32_t kMaxSpans = 8;
struct FlagSpans {
    uint32_t n_spans;
    uint32_t first_block[kMaxSpans + 1];
    uint64_t offset[kMaxSpans], n[kMaxSpans];
    uint32_t slot[kMaxSpans];
};
template <typename GT>
__global__ void __launch_bounds__(256)
k_nonfinite_flag(FlagSpans r, const GT* __restrict__ g, uint32_t* __restrict__ flags) {
    uint32_t k = 0;
    while (k + 1 < r.n_spans && blockIdx.x >= r.first_block[k + 1]) ++k;
    const bool bad = nonfinite_range<GT>(r.n[k], g + r.offset[k], blockIdx.x - r.first_block[k],
                                         r.first_block[k + 1] - r.first_block[k]);
    if (__ballot(bad) != 0ull && (threadIdx.x & 63) == 0) atomicOr(flags + r.slot[k], 1u);
}

__global__ void __launch_bounds__(256)
k_cast_half(uint64_t n, const float* __restrict__ src, _Float16* __restrict__ dst) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool aligned = (((uintptr_t)src & 15u) | ((uintptr_t)dst & 7u)) == 0u;
    const uint64_t n_vec = aligned ? n / 4 : 0u;
    for (uint64_t i = tid; i < n_vec; i += stride) {
        const float4 v = reinterpret_cast<const float4*>(src)[i];
        typedef _Float16 h4v __attribute__((ext_vector_type(4)));
        reinterpret_cast<h4v*>(dst)[i] = h4v{(_Float16)v.x, (_Float16)v.y, (_Float16)v.z, (_Float16)v.w};
    }
    for (uint64_t i = n_vec * 4 + tid; i < n; i += stride) dst[i] = (_Float16)src[i];
}

// fp32 -> 16-bit working copy in the mixed format of Copy16Fmt
__global__ void __launch_bounds__(256)
k_cast_working_copy(uint64_t n, const float* __restrict__ src, nvo_h16* __restrict__ dst, Copy16Fmt fmt) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        dst[i] = nvo_cvt16(src[i], fmt.is_bf16(i));
}

__global__ void __launch_bounds__(256)
k_cast_bf16(uint64_t n, const float* __restrict__ src, uint16_t* __restrict__ dst) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool aligned = (((uintptr_t)src & 15u) | ((uintptr_t)dst & 7u)) == 0u;
    const uint64_t n_vec = aligned ? n / 4 : 0u;
    for (uint64_t i = tid; i < n_vec; i += stride) {
        const float4 v = reinterpret_cast<const float4*>(src)[i];
        reinterpret_cast<uint2*>(dst)[i] = make_uint2((uint32_t)to_bf16(v.x) | ((uint32_t)to_bf16(v.y) << 16),
                                                      (uint32_t)to_bf16(v.z) | ((uint32_t)to_bf16(v.w) << 16));
    }
    for (uint64_t i = n_vec * 4 + tid; i < n; i += stride) dst[i] = to_bf16(src[i]);
}

// ---- sharded gradient exchange (reduce-scatter -> Adam on this rank's 1/W slice -> all-gather of the working copy) ----
// The fp32 gradient range [0, n) is cast to the 2-byte wire format as W chunks of `per` elements, each followed by `pad`
// FLAG slots: wire[(i / per) * (per + pad) + i % per] = cvt(src[i]).  A non-finite source value raises *flag (the rank's
// LOCAL overflow flag).  k_flag_to_wire then writes flag ? 1 : 0 into every chunk's pad slots, so that after the SUM
// reduce-scatter rank r finds the number of ranks that overflowed in the pad of ITS chunk -- every rank learns the same
// verdict without a second collective (GradScaler.step must skip the whole group everywhere or nowhere).
template <bool BF>
__global__ void __launch_bounds__(256)
k_cast_shards(uint64_t n, uint64_t per, uint32_t pad, const float* __restrict__ src, uint16_t* __restrict__ dst,
              uint32_t* __restrict__ flag) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool bad = false;
    auto cvt = [](float x) -> uint16_t {
        if (BF) return to_bf16(x);
        return __builtin_bit_cast(uint16_t, (_Float16)x);
    };
    // per and pad are multiples of 4 (checked on the host): a 4-vector never straddles a chunk
    for (uint64_t q = tid; q < n / 4; q += stride) {
        const uint64_t i = q * 4;
        const float4 v = reinterpret_cast<const float4*>(src)[q];
        // (what does not survive the cast -- beyond 65504 on an fp16 wire -- counts as an overflow as well; and on that
        // wire the SUM of `world` finite addends must stay finite too, since nothing scans the reduced shard: a rank
        // whose own value exceeds 65504 / world raises the flag, which keeps the verdict global -- the flag slots are
        // summed with the gradient -- and the loss scale identical on all ranks.  bf16 has fp32's range.)
        const float lim = BF ? 3.0e38f : 65504.0f / (float)(n / per);
        bad = bad || !(fabsf(v.x) <= lim) || !(fabsf(v.y) <= lim) || !(fabsf(v.z) <= lim) || !(fabsf(v.w) <= lim);
        const uint64_t o = (i / per) * (per + pad) + (i % per);
        *reinterpret_cast<uint2*>(dst + o) = make_uint2((uint32_t)cvt(v.x) | ((uint32_t)cvt(v.y) << 16),
                                                        (uint32_t)cvt(v.z) | ((uint32_t)cvt(v.w) << 16));
    }
    if (flag && __ballot(bad) != 0ull && (threadIdx.x & 63) == 0) atomicOr(flag, 1u);
}

template <bool BF>
__global__ void k_flag_to_wire(const uint32_t* __restrict__ flag, uint16_t* __restrict__ wire, uint64_t per, uint32_t pad,
                               uint32_t world) {
    const uint16_t one = BF ? (uint16_t)0x3F80u : (uint16_t)0x3C00u;
    const uint16_t v = *flag ? one : (uint16_t)0;
    for (uint32_t t = threadIdx.x; t < world * pad; t += blockDim.x)
        wire[(uint64_t)(t / pad) * (per + pad) + per + (t % pad)] = v;
}

__global__ void k_flag_from_wire(const uint16_t* __restrict__ slot, uint32_t* __restrict__ flag) {
    if (threadIdx.x == 0 && (slot[0] & 0x7FFFu) != 0u) atomicOr(flag, 1u);  // any non-zero count (or a NaN) = overflow
}

// tcnn EmaOptimizer::step [UPSTREAM, restated]: the debiased exponential moving average of the weights,
//   ema_t = (ema_{t-1} * decay * (1 - decay^(t-1)) + w_t * (1 - decay)) / (1 - decay^t),
// kept in fp32 with a 16-bit copy for inference.  skip_flag (the optimiser's): non-zero = the step was skipped, the
// average keeps its value.
// t = *step_dev + 1, the step count kept on the device: *step_dev = number of averages APPLIED so far; a skipped optimiser
// step leaves both the average and the counter alone (k_ema_commit), so the debias factor 1 / (1 - decay^t) never runs
// ahead of the average it normalises
__global__ void __launch_bounds__(256)
k_ema_update(uint64_t n, const float* __restrict__ params, float* __restrict__ ema, _Float16* __restrict__ ema_half,
                 float decay, const uint32_t* __restrict__ step_dev, const uint32_t* __restrict__ skip_flag) {
    if (skip_flag && skip_flag[0] != 0u) return;
    __shared__ float fac[2];
    if (threadIdx.x == 0) {
        const double d = (double)decay, t = (double)(*step_dev) + 1.0;
        fac[0] = (float)(d * (1.0 - pow(d, t - 1.0)));
        fac[1] = (float)(1.0 / (1.0 - pow(d, t)));
    }
    __syncthreads();
    const float keep = fac[0], inv_debias = fac[1], take = 1.0f - decay;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    // pure stream (8 B read + 6 B written per weight): 16-byte accesses when the buffers allow it
    uint64_t done = 0;
    if (((((uintptr_t)params) | ((uintptr_t)ema)) & 15u) == 0u && (((uintptr_t)ema_half) & 7u) == 0u) {
        const uint64_t n4 = n >> 2;
        for (uint64_t q = tid; q < n4; q += stride) {
            const float4 pv = reinterpret_cast<const float4*>(params)[q];
            float4 ev = reinterpret_cast<float4*>(ema)[q];
            ev.x = (ev.x * keep + pv.x * take) * inv_debias;
            ev.y = (ev.y * keep + pv.y * take) * inv_debias;
            ev.z = (ev.z * keep + pv.z * take) * inv_debias;
            ev.w = (ev.w * keep + pv.w * take) * inv_debias;
            reinterpret_cast<float4*>(ema)[q] = ev;
            if (ema_half) {
                *reinterpret_cast<uint2*>(ema_half + (q << 2)) =
                    make_uint2(nvo_cvt16x2(ev.x, ev.y, false), nvo_cvt16x2(ev.z, ev.w, false));
            }
        }
        done = n4 << 2;
    }
    for (uint64_t i = done + tid; i < n; i += stride) {
        const float e = (ema[i] * keep + params[i] * take) * inv_debias;
        ema[i] = e;
        if (ema_half) ema_half[i] = __builtin_bit_cast(_Float16, nvo_cvt16(e, false));  // (fp32 first, then fp16: as above)
    }
}
__global__ void k_ema_commit(uint32_t* __restrict__ step_dev, const uint32_t* __restrict__ skip_flag) {
    if (threadIdx.x == 0 && blockIdx.x == 0 && !(skip_flag && skip_flag[0] != 0u)) *step_dev += 1u;
}

// GradScaler.update() + the optimisers' step counters, on the device (one thread): group i of `active_mask` advances its
// applied-step counter iff its skip flag is clear; the loss scale backs off when ANY active group saw a non-finite
// gradient and grows after `interval` clean steps (torch.cuda.amp.GradScaler: init 65536, x2 / 2000 steps, x0.5).
__device__ void opt_commit_thread(uint32_t n_groups, uint32_t active_mask, uint32_t scale_mask, uint32_t* __restrict__ applied,
                             const uint32_t* __restrict__ skip_flags, float* __restrict__ scale,
                             uint32_t* __restrict__ growth_tracker, float growth, float backoff, uint32_t interval,
                             float min_scale, float max_scale, float* __restrict__ bias, float beta1, float beta2) {
    bool any_bad = false;
    for (uint32_t i = 0; i < n_groups; ++i) {
        const bool bad = skip_flags && skip_flags[i] != 0u;
        if ((scale_mask >> i) & 1u) any_bad = any_bad || bad;
        if (((active_mask >> i) & 1u) && applied && !bad) {
            const uint32_t done = applied[i] + 1u;
            applied[i] = done;
            if (bias) {  // bias corrections of the group's NEXT applied step (double: 1 - 0.999^t loses digits in fp32)
                const double t = (double)done + 1.0;
                bias[2 * i + 0] = (float)(1.0 - pow((double)beta1, t));
                bias[2 * i + 1] = (float)sqrt(1.0 - pow((double)beta2, t));
            }
        }
    }
    if (scale) {
        float sc = *scale;
        uint32_t tr = *growth_tracker;
        if (any_bad) {
            sc = fmaxf(sc * backoff, min_scale);
            tr = 0u;
        } else if (++tr >= interval) {
            sc = fminf(sc * growth, max_scale);
            tr = 0u;
        }
        *scale = sc;
        *growth_tracker = tr;
    }
}

struct NvoFloats16 { float v[16]; };
__global__ void k_write_floats(float* dst, uint32_t n, NvoFloats16 vals) {
    if (threadIdx.x < n) dst[threadIdx.x] = vals.v[threadIdx.x];
}

// GradScaler.update / step counters of the step that just ran and, with n != 0, the per-step scalars of the next one
// in ONE tiny eager launch: a graph-replayed step ends with its Adam launch, the commit rides in the launch that every
// step needs anyway for its scalars (one dependent 5-us launch less per step).
__global__ void k_opt_commit(nvo_opt_commit_args a, float* dst, uint32_t n, NvoFloats16 vals) {
    if (threadIdx.x < n) dst[threadIdx.x] = vals.v[threadIdx.x];
    if (threadIdx.x == 63)
        opt_commit_thread(a.n_groups, a.active_mask, a.scale_mask, a.applied, a.skip_flags, a.scale, a.growth_tracker,
                          a.growth_factor, a.backoff_factor, a.growth_interval, a.min_scale, a.max_scale, a.bias, a.beta1, a.beta2);
}

// The same commit as a node INSIDE the captured step: the per-step scalars of the next step come from a device table the
// host fills ahead (row s % table_rows = the 16 scalars of step s) and a device step counter the kernel advances -- no
// eager launch behind the replay (measured: 8 us of launch latency between the graph's last kernel and the eager one,
// plus its 5 us, on every step).
__global__ void k_opt_commit_table(uint32_t n_groups, uint32_t active_mask, uint32_t scale_mask, uint32_t* __restrict__ applied,
                                   const uint32_t* __restrict__ skip_flags, float* __restrict__ scale,
                                   uint32_t* __restrict__ growth_tracker, float growth, float backoff, uint32_t interval,
                                   float min_scale, float max_scale, float* __restrict__ bias, float beta1, float beta2,
                                   float* dst, const float* __restrict__ table, uint32_t table_rows,
                                   uint32_t* __restrict__ next_step) {
    const uint32_t s = *next_step;
    if (threadIdx.x < 16) dst[threadIdx.x] = table[(size_t)(s % table_rows) * 16u + threadIdx.x];
    if (threadIdx.x == 63)
        opt_commit_thread(n_groups, active_mask, scale_mask, applied, skip_flags, scale, growth_tracker, growth, backoff, interval,
                          min_scale, max_scale, bias, beta1, beta2);
    __syncthreads();
    if (threadIdx.x == 0) *next_step = s + 1u;
}

int make_copy_fmt(uint32_t n_ranges, const uint64_t* lo, const uint64_t* hi, Copy16Fmt* fmt) {
    NVO_REQUIRE(n_ranges <= kMaxBf16Ranges && (n_ranges == 0 || (lo && hi)), "working copy: at most %u bf16 ranges",
                kMaxBf16Ranges);
    memset(fmt, 0, sizeof(*fmt));
    fmt->n = n_ranges;
    for (uint32_t k = 0; k < n_ranges; ++k) {
        NVO_REQUIRE((lo[k] & 3u) == 0 && (hi[k] & 3u) == 0 && lo[k] <= hi[k], "working copy: bf16 range %u is not 4-aligned", k);
        fmt->lo[k] = lo[k];
        fmt->hi[k] = hi[k];
    }
    return NVO_OK;
}

// the one validation of nvo_opt_commit_args: nvo_opt_commit and the commit a nvo_adam_tail carries
int check_commit_args(const nvo_opt_commit_args& a, const char* who) {
    NVO_REQUIRE(a.n_groups >= 1 && a.n_groups <= kAdamMaxGroups, "%s: 1..%u commit groups (got %u)", who, kAdamMaxGroups,
                a.n_groups);
    NVO_REQUIRE(a.applied || a.scale, "%s: nothing to update", who);
    NVO_REQUIRE(!a.scale || (a.growth_tracker && a.growth_interval >= 1 && a.growth_factor >= 1.f && a.backoff_factor > 0.f &&
                             a.backoff_factor <= 1.f && a.min_scale > 0.f && a.max_scale >= a.min_scale),
                "%s: bad loss-scale schedule", who);
    return NVO_OK;
}

}  // namespace

extern "C" {

int nvo_adam_step(nvo_stream_t stream, const nvo_adam_args* args, uint32_t n_groups, const nvo_adam_group* groups,
                  const nvo_adam_tail* tail) {
    NVO_REQUIRE(args && groups, "adam_step: NULL argument");
    const nvo_adam_args& a = *args;
    NVO_REQUIRE(a.params && a.grads && a.exp_avg && a.exp_avg_sq, "adam_step: NULL buffer");
    NVO_REQUIRE(a.grads_fmt >= 0 && a.grads_fmt <= 2, "adam_step: grads_fmt 0 (fp32), 1 (fp16) or 2 (bf16)");
    nvo_adam_tail t{};
    if (tail) {
        t = *tail;
        NVO_REQUIRE(!t.ema || (t.ema_step_dev && t.ema_decay >= 0.f && t.ema_decay < 1.f && t.ema_flag_slot < kAdamMaxGroups),
                    "adam_step: the tail's weight average needs its step counter, 0 <= decay < 1");
        const bool opt_commit = t.commit.applied || t.commit.scale;
        if (opt_commit) {
            if (int rc = check_commit_args(t.commit, "adam_step tail")) return rc;
            // (the last workgroup commits with the flags and betas the launch itself read)
            NVO_REQUIRE(t.commit.skip_flags == a.skip_flags && t.commit.beta1 == a.beta1 && t.commit.beta2 == a.beta2,
                        "adam_step: the tail's commit must name the launch's skip_flags, beta1 and beta2");
        }
        if (!t.ema) t.ema_commit = 0u;
        const bool commit = opt_commit || t.ema_commit;
        NVO_REQUIRE(!commit || t.done_counter, "adam_step: the tail's commit needs done_counter (a zeroed device word)");
        if (!commit) t.done_counter = nullptr;  // (no check-in)
    }
    Copy16Fmt fmt;
    if (int rc = make_copy_fmt(a.n_bf16_ranges, a.bf16_lo, a.bf16_hi, &fmt)) return rc;
    NVO_REQUIRE(n_groups >= 1 && n_groups <= kAdamMaxGroups, "adam_step: 1..%u groups (got %u)", kAdamMaxGroups, n_groups);
    NVO_PROF(stream, "adam");
    AdamGroups gr{};
    uint32_t k = 0, blocks_total = 0;
    const size_t gsz = a.grads_fmt ? 2 : 4;
    for (uint32_t i = 0; i < n_groups; ++i) {
        if (groups[i].n == 0) continue;
        NVO_REQUIRE(groups[i].step >= 1 || groups[i].bias_dev, "adam_step: step counts from 1");
        NVO_REQUIRE(groups[i].flag_slot < kAdamMaxGroups, "adam_step: flag_slot %u out of range", groups[i].flag_slot);
        const uint64_t o = groups[i].offset;
        gr.offset[k] = o;
        gr.n[k] = groups[i].n;
        gr.lr[k] = groups[i].lr;
        nvo_host_bias_pair(a.beta1, a.beta2, groups[i].step, &gr.bias1[k], &gr.bias2_sqrt[k]);
        gr.hyper_dev[k] = groups[i].hyper_dev;
        gr.bias_dev[k] = groups[i].bias_dev;
        gr.slot[k] = groups[i].flag_slot;
        gr.wd[k] = groups[i].weight_decay;
        const uintptr_t align = (uintptr_t)(a.params + o) | (uintptr_t)(a.exp_avg + o) | (uintptr_t)(a.exp_avg_sq + o);
        gr.vec4[k] = (align & 15u) == 0 && (!a.params_half || (((uintptr_t)a.params_half + 2 * o) & 7u) == 0) &&
                     ((((uintptr_t)a.grads + gsz * o) & (a.grads_fmt ? 7u : 15u)) == 0);
        uint32_t blocks = nvo_div_up(groups[i].n, 256 * 8);
        if (blocks > 4096) blocks = 4096;
        gr.first_block[k] = blocks_total;
        blocks_total += blocks;
        ++k;
    }
    NVO_REQUIRE(k > 0 || !(t.done_counter || t.ema), "adam_step: a tail needs at least one non-empty group");
    if (k == 0) return NVO_OK;
    gr.n_groups = k;
    for (uint32_t i = k; i <= kAdamMaxGroups; ++i) gr.first_block[i] = blocks_total;
    if (t.ema) {
        // (the 16-byte form of a group reads the average like the parameters: same alignment or the scalar form)
        for (uint32_t i = 0; i < k; ++i) {
            const uintptr_t al = (uintptr_t)(t.ema + gr.offset[i]);
            if ((al & 15u) != 0 || (t.ema_half && (((uintptr_t)t.ema_half + 2 * gr.offset[i]) & 7u) != 0)) gr.vec4[i] = 0;
        }
    }
    AdamHyper h{0.f, a.beta1, a.beta2, a.eps, 1.f, 1.f, a.grad_scale, 0.f};  // (lr, bias corrections, decay: per group)
    if (a.grads_fmt == 2) {
        NVO_LAUNCH(k_adam_groups<Bf16>, dim3(blocks_total), dim3(256), 0, (hipStream_t)stream, gr, a.params,
                   (nvo_h16*)a.params_half, (const Bf16*)a.grads, a.exp_avg, a.exp_avg_sq, h, a.skip_flags, fmt,
                   a.loss_scale_dev, t);
    } else if (a.grads_fmt) {
        NVO_LAUNCH(k_adam_groups<_Float16>, dim3(blocks_total), dim3(256), 0, (hipStream_t)stream, gr, a.params,
                   (nvo_h16*)a.params_half, (const _Float16*)a.grads, a.exp_avg, a.exp_avg_sq, h, a.skip_flags, fmt,
                   a.loss_scale_dev, t);
    } else {
        NVO_LAUNCH(k_adam_groups<float>, dim3(blocks_total), dim3(256), 0, (hipStream_t)stream, gr, a.params,
                   (nvo_h16*)a.params_half, (const float*)a.grads, a.exp_avg, a.exp_avg_sq, h, a.skip_flags, fmt,
                   a.loss_scale_dev, t);
    }
    NVO_CHECK_LAUNCH();
    return NVO_OK;
}

int nvo_opt_commit(nvo_stream_t stream, const nvo_opt_commit_args* args, const nvo_step_scalars* scalars) {
    NVO_REQUIRE(args, "opt_commit: NULL argument");
    const nvo_opt_commit_args& a = *args;
    if (int rc = check_commit_args(a, "opt_commit")) return rc;
    if (scalars && scalars->table) {
        const nvo_step_scalars& s = *scalars;
        NVO_REQUIRE(s.dst && !s.host_values && s.n == 16 && s.next_step && s.table_rows >= 1,
                    "opt_commit: the scalar table form needs dst, next_step, rows of n == 16 and no host_values");
        NVO_LAUNCH(k_opt_commit_table, dim3(1), dim3(64), 0, (hipStream_t)stream, a.n_groups, a.active_mask, a.scale_mask,
                   a.applied, a.skip_flags, a.scale, a.growth_tracker, a.growth_factor, a.backoff_factor, a.growth_interval,
                   a.min_scale, a.max_scale, a.bias, a.beta1, a.beta2, s.dst, s.table, s.table_rows, s.next_step);
    } else {
        NvoFloats16 vals{};
        const uint32_t n = scalars ? scalars->n : 0u;
        NVO_REQUIRE(!scalars || (scalars->dst && scalars->host_values && n <= 16), "opt_commit: bad scalar block (n <= 16)");
        for (uint32_t i = 0; i < n; ++i) vals.v[i] = scalars->host_values[i];
        NVO_LAUNCH(k_opt_commit, dim3(1), dim3(64), 0, (hipStream_t)stream, a, scalars ? scalars->dst : nullptr, n, vals);
    }
    NVO_CHECK_LAUNCH();
    return NVO_OK;
}

int nvo_nonfinite_flag(nvo_stream_t stream, uint32_t n_spans, const uint64_t* offsets, const uint64_t* sizes,
                       const uint32_t* slots, const void* grads, int grads_fmt, uint32_t* flags, int reset) {
    NVO_REQUIRE(grads && flags && offsets && sizes, "nonfinite_flag: NULL argument");
    NVO_REQUIRE(n_spans >= 1 && n_spans <= kMaxSpans, "nonfinite_flag: 1..%u spans (got %u)", kMaxSpans, n_spans);
    NVO_REQUIRE(grads_fmt >= 0 && grads_fmt <= 2, "nonfinite_flag: grads_fmt 0 (fp32), 1 (fp16) or 2 (bf16)");
    NVO_REQUIRE(!(reset && slots), "nonfinite_flag: reset clears flags[0..n_spans), which explicit slots do not name");
    NVO_PROF(stream, "nonfinite_flag");
    if (reset)
        if (int rc = nvo_zero_async(flags, sizeof(uint32_t) * n_spans, (hipStream_t)stream)) return rc;
    FlagSpans r{};
    uint32_t k = 0, blocks_total = 0;
    for (uint32_t i = 0; i < n_spans; ++i) {
        if (sizes[i] == 0) continue;
        r.offset[k] = offsets[i];
        r.n[k] = sizes[i];
        r.slot[k] = slots ? slots[i] : i;
        uint32_t blocks = nvo_div_up(sizes[i], 256 * 8);
        if (blocks > 2048) blocks = 2048;
        r.first_block[k] = blocks_total;
        blocks_total += blocks;
        ++k;
    }
    if (k == 0) return NVO_OK;
    r.n_spans = k;
    for (uint32_t i = k; i <= kMaxSpans; ++i) r.first_block[i] = blocks_total;
    if (grads_fmt == 2) {
        NVO_LAUNCH(k_nonfinite_flag<Bf16>, dim3(blocks_total), dim3(256), 0, (hipStream_t)stream, r, (const Bf16*)grads, flags);
    } else if (grads_fmt) {
        NVO_LAUNCH(k_nonfinite_flag<_Float16>, dim3(blocks_total), dim3(256), 0, (hipStream_t)stream, r, (const _Float16*)grads,
                   flags);
    } else {
        NVO_LAUNCH(k_nonfinite_flag<float>, dim3(blocks_total), dim3(256), 0, (hipStream_t)stream, r, (const float*)grads, flags);
    }
    NVO_CHECK_LAUNCH();
    return NVO_OK;
}

int nvo_write_floats(nvo_stream_t stream, float* dst, uint32_t n, const float* host_values) {
    NVO_REQUIRE(dst && host_values && n <= 16, "write_floats: bad argument (n <= 16)");
    if (n == 0) return NVO_OK;
    NvoFloats16 vals;
    for (uint32_t i = 0; i < 16; ++i) vals.v[i] = i < n ? host_values[i] : 0.f;
    NVO_LAUNCH(k_write_floats, dim3(1), dim3(64), 0, (hipStream_t)stream, dst, n, vals);  // values travel by value
    NVO_CHECK_LAUNCH();
    return NVO_OK;
}

int nvo_ema_update(nvo_stream_t stream, uint64_t n, const float* params, float* ema, void* ema_half, float decay,
                   uint32_t* step_dev, const uint32_t* skip_flag, int commit) {
    NVO_REQUIRE(params && ema && step_dev, "ema_update: NULL argument");
    NVO_REQUIRE(decay >= 0.f && decay < 1.f, "ema_update: 0 <= decay < 1");
    if (n == 0) return NVO_OK;
    NVO_PROF(stream, "ema_update");
    uint32_t blocks = nvo_div_up(n, 256 * 4);
    if (blocks > 2048) blocks = 2048;
    NVO_LAUNCH(k_ema_update, dim3(blocks), dim3(256), 0, (hipStream_t)stream, n, params, ema, (_Float16*)ema_half, decay,
               (const uint32_t*)step_dev, skip_flag);
    if (commit) NVO_LAUNCH(k_ema_commit, dim3(1), dim3(64), 0, (hipStream_t)stream, step_dev, skip_flag);
    NVO_CHECK_LAUNCH();
    return NVO_OK;
}

int nvo_cast_working_copy(nvo_stream_t stream, uint64_t n, const float* src, void* dst16, uint32_t n_bf16_ranges,
                          const uint64_t* bf16_lo, const uint64_t* bf16_hi) {
    NVO_REQUIRE(src && dst16, "cast_working_copy: NULL argument");
    Copy16Fmt fmt;
    if (int rc = make_copy_fmt(n_bf16_ranges, bf16_lo, bf16_hi, &fmt)) return rc;
    if (n == 0) return NVO_OK;
    NVO_PROF(stream, "cast_half");
    uint32_t blocks = nvo_div_up(n, 256 * 4);
    if (blocks > 2048) blocks = 2048;
    NVO_LAUNCH(k_cast_working_copy, dim3(blocks), dim3(256), 0, (hipStream_t)stream, n, src, (nvo_h16*)dst16, fmt);
    NVO_CHECK_LAUNCH();
    return NVO_OK;
}

int nvo_cast_bf16(nvo_stream_t stream, uint64_t n, const float* src, void* dst_bf16) {
    NVO_REQUIRE(src && dst_bf16, "cast_bf16: NULL argument");
    if (n == 0) return NVO_OK;
    NVO_PROF(stream, "cast_bf16");
    uint32_t blocks = nvo_div_up(n, 256 * 4);
    if (blocks > 2048) blocks = 2048;
    NVO_LAUNCH(k_cast_bf16, dim3(blocks), dim3(256), 0, (hipStream_t)stream, n, src, (uint16_t*)dst_bf16);
    NVO_CHECK_LAUNCH();
    return NVO_OK;
}

int nvo_cast_shards(nvo_stream_t stream, uint64_t n, uint32_t world, uint32_t pad, const float* src, void* wire16,
                    int wire_fmt, uint32_t* flag) {
    NVO_REQUIRE(src && wire16 && flag, "cast_shards: NULL argument");
    NVO_REQUIRE(world >= 1 && n % ((uint64_t)world * 4) == 0 && pad % 4 == 0 && pad >= 4,
                "cast_shards: n (%llu) must be a multiple of 4 x world (%u), pad (%u) a positive multiple of 4",
                (unsigned long long)n, world, pad);
    NVO_REQUIRE(wire_fmt == 1 || wire_fmt == 2, "cast_shards: wire format 1 (fp16) or 2 (bf16)");
    NVO_REQUIRE((((uintptr_t)src & 15u) | ((uintptr_t)wire16 & 7u)) == 0, "cast_shards: unaligned buffers");
    if (n == 0) return NVO_OK;
    const uint64_t per = n / world;
    NVO_PROF(stream, "cast_shards");
    uint32_t blocks = nvo_div_up(n, 256 * 4 * 4);
    if (blocks > 2048) blocks = 2048;
    if (wire_fmt == 2) {
        NVO_LAUNCH(k_cast_shards<true>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, n, per, pad, src, (uint16_t*)wire16, flag);
        NVO_LAUNCH(k_flag_to_wire<true>, dim3(1), dim3(64), 0, (hipStream_t)stream, flag, (uint16_t*)wire16, per, pad, world);
    } else {
        NVO_LAUNCH(k_cast_shards<false>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, n, per, pad, src, (uint16_t*)wire16, flag);
        NVO_LAUNCH(k_flag_to_wire<false>, dim3(1), dim3(64), 0, (hipStream_t)stream, flag, (uint16_t*)wire16, per, pad, world);
    }
    NVO_CHECK_LAUNCH();
    return NVO_OK;
}

int nvo_flag_from_wire(nvo_stream_t stream, const void* wire_slot16, uint32_t* flag) {
    NVO_REQUIRE(wire_slot16 && flag, "flag_from_wire: NULL argument");
    NVO_LAUNCH(k_flag_from_wire, dim3(1), dim3(64), 0, (hipStream_t)stream, (const uint16_t*)wire_slot16, flag);
    NVO_CHECK_LAUNCH();
    return NVO_OK;
}

int nvo_cast_half(nvo_stream_t stream, uint64_t n, const float* src, void* dst_half) {
    NVO_REQUIRE(src && dst_half, "cast_half: NULL argument");
    if (n == 0) return NVO_OK;
    NVO_PROF(stream, "cast_half");
    uint32_t blocks = nvo_div_up(n, 256 * 4);
    if (blocks > 2048) blocks = 2048;
    NVO_LAUNCH(k_cast_half, dim3(blocks), dim3(256), 0, (hipStream_t)stream, n, src,
                       (_Float16*)dst_half);
    NVO_CHECK_LAUNCH();
    return NVO_OK;
}

}  // extern "C"
