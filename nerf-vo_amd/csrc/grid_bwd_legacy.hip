// The slice-owner backward (k_grid_bwd_lds / grid_bwd_item of grid.hip) as it stood BEFORE its scans were made
// instruction-lean: verbatim copies (only the names carry a _legacy suffix), kept as the A/B and same-bits reference
// behind the module option "grid_bwd_scan" = 0 (tests/test_grid_bwd_lean_gpu.py, EXPERIMENTS.md 12.5).  Not a product
// path.  The launcher of grid.hip prepares everything (item table, L1 norms, live list, ring offset) and only the choice
// of the kernel is made here, on the host.
#include "nvo_kernels.h"

#include <math.h>

#define GP_CLK(v) do { } while (0)
#define GP_ADD(slot, d) do { } while (0)

namespace {

// dL/d(encoded) pair of one (sample, level): fp16 (tcnn's precision), fp32, or bfloat16 (bf16 MLP mode)
struct Bf2 {
    uint32_t raw;
};
__device__ __forceinline__ float2 dy2f(__half2 v) { return __half22float2(v); }
__device__ __forceinline__ float2 dy2f(float2 v) { return v; }
__device__ __forceinline__ float2 dy2f(Bf2 v) {
    return make_float2(__uint_as_float(v.raw << 16), __uint_as_float(v.raw & 0xFFFF0000u));
}

struct Corner {
    uint32_t px, py, pz;  // cell base
    float wx, wy, wz;     // fractional position
};

__device__ __forceinline__ Corner grid_cell(float scale, float x, float y, float z) {
    // tcnn pos_fract: pos = fma(scale, x, 0.5); cell = floor(pos); frac = pos - cell.
    Corner c;
    float fx = fmaf(scale, x, 0.5f), fy = fmaf(scale, y, 0.5f), fz = fmaf(scale, z, 0.5f);
    float tx = floorf(fx), ty = floorf(fy), tz = floorf(fz);
    c.px = (uint32_t)(int)tx;
    c.py = (uint32_t)(int)ty;
    c.pz = (uint32_t)(int)tz;
    c.wx = fx - tx;
    c.wy = fy - ty;
    c.wz = fz - tz;
    return c;
}

constexpr uint32_t kSliceFixed = 8192;
constexpr uint32_t kSliceFloat = 20448;  // (160 KiB less 256 B: the item's work counter is static LDS)
constexpr uint32_t kLdsBwdBytes = 160 * 1024;
constexpr int kLdsBwdBlock = 1024;
constexpr uint32_t kHitCap = 127;
constexpr float kFixScale = 67108864.f;          // 2^26
constexpr float kFixInv = 1.0f / 67108864.f;

// float -> 2^26 fixed point through the double "magic number" trick: (double)v * 2^26 + 1.5 * 2^52
// leaves round-to-nearest(v * 2^26) in the low mantissa bits, so one cvt + one f64 fma + a 64-bit
// subtract replace the ~20-instruction software float->int64 conversion.  Valid for |v| < 2^25.
__device__ __forceinline__ unsigned long long to_fixed(float v) {
    const double magic = 6755399441055744.0;  // 1.5 * 2^52
    const double t = fma((double)v, (double)kFixScale, magic);
    return (unsigned long long)(__double_as_longlong(t) - __double_as_longlong(magic));
}

// Per-item scale context of the accumulators (only AccFixed32 uses it): s = fixed-point scale per feature,
// inv = its reciprocal.
struct AccScale {
    float s0, s1, inv0, inv1;
};

struct AccFixed {
    typedef unsigned long long T;
    static constexpr uint32_t kEntries = kSliceFixed;
    static __device__ __forceinline__ void add(T* acc, uint32_t rel, float v0, float v1, const AccScale&) {
        atomicAdd(&acc[2 * rel + 0], to_fixed(v0));
        atomicAdd(&acc[2 * rel + 1], to_fixed(v1));
    }
    // int64 -> float through double (cvt_f64_i32 + cvt_f64_u32 + one f64 fma + cvt_f32_f64: 4 instructions instead of
    // the ~12 of the software int64 -> float conversion; the double holds every |sum| < 2^53 -- 1.3e8 in gradient
    // units -- exactly, so the one rounding to float is the correctly rounded conversion)
    static __device__ __forceinline__ float get(const T* acc, uint32_t e, const AccScale&) {
        const unsigned long long v = acc[e];
        const double d = fma((double)(int)(uint32_t)(v >> 32), 4294967296.0, (double)(uint32_t)v);
        return (float)d * kFixInv;
    }
};
struct AccFloat {
    typedef float T;
    static constexpr uint32_t kEntries = kSliceFloat;
    static __device__ __forceinline__ void add(T* acc, uint32_t rel, float v0, float v1, const AccScale&) {
        atomicAdd(&acc[2 * rel + 0], v0);
        atomicAdd(&acc[2 * rel + 1], v1);
    }
    static __device__ __forceinline__ float get(const T* acc, uint32_t e, const AccScale&) { return acc[e]; }
};
// 32-bit fixed point with a DATA-DERIVED, overflow-proof scale: every contribution to an entry is w * dy with
// trilinear weights 0 <= w <= 1 that sum to 1 over a sample's corners, so |sum| <= L1_f = sum_i |dy_f(i)| of
// the level for any entry; scale_f = 2^29 / L1_f keeps every partial sum (rounding slack included) inside
// int32.  Resolution L1_f / 2^29 -- relative ~1e-5..1e-4 for a typical entry of a coarse level, i.e. finer
// than the fp16 accumulation of the reference (2^-11 per add) though coarser than the 64-bit form.  Half the
// LDS per entry => 16K-entry slices => half the slices of a level (half the redundant scans), a 2-instruction
// conversion instead of cvt_f64 + fma_f64 + 64-bit subtract, and 32-bit LDS atomics.  Integer adds are
// associative: results are bitwise reproducible for single-chunk items.
struct AccFixed32 {
    typedef int T;
    static constexpr uint32_t kEntries = 16384;
    static __device__ __forceinline__ void add(T* acc, uint32_t rel, float v0, float v1, const AccScale& sc) {
        atomicAdd(&acc[2 * rel + 0], __float2int_rn(v0 * sc.s0));
        atomicAdd(&acc[2 * rel + 1], __float2int_rn(v1 * sc.s1));
    }
    static __device__ __forceinline__ float get(const T* acc, uint32_t e, const AccScale& sc) {
        return (float)acc[e] * ((e & 1u) ? sc.inv1 : sc.inv0);
    }
};

// One workgroup per WORK ITEM = (level, slice, sample chunk).  A slice of a large hashed level is
// hit by a small share of all corner lookups and gets one item that scans every sample and writes
// its slice with plain stores.  A slice that is hit often (dense levels, small tables) is split into
// sample chunks of equal expected hit count (table built on the host from the hit share alone,
// independent of N); chunked items flush with row-contiguous float atomics (256-B shaped, the fast
// form) into a pre-zeroed range.
template <typename ACC, bool SOA, typename DY2>
__device__ __forceinline__ void grid_bwd_item_legacy(const NvoGridLevels& g, uint32_t N,
                                              const float* __restrict__ x, const DY2* __restrict__ dy,
                                              float* __restrict__ grad, uint32_t level, uint32_t first,
                                              uint32_t chunk, uint32_t n_chunks, void* lds_raw,
                                              const AccScale sc = AccScale{0.f, 0.f, 0.f, 0.f},
                                              const uint32_t* __restrict__ live = nullptr, bool merge = false,
                                              uint32_t slice_cap = ACC::kEntries, uint32_t* __restrict__ nf_flag = nullptr,
                                              const uint32_t* __restrict__ live_n = nullptr, uint32_t ring_off = 0u,
                                              uint32_t list_pass = 4096u) {
    typename ACC::T* acc = reinterpret_cast<typename ACC::T*>(lds_raw);
    const uint32_t off = g.offset[level];
    const uint32_t size = g.offset[level + 1] - off;
    const uint32_t res = g.resolution[level];
    const uint32_t hashed = g.hashed[level];
    const float scale = g.scale[level];
    const uint32_t count = min(slice_cap, size - first);  // slice_cap <= ACC::kEntries
    // live != nullptr: *live_n = number of samples with a non-zero gradient, live[j] = their ids; the chunks then
    // partition that list.  (A list that holds most of the samples is not worth the indirection: identity scan.)
    const uint32_t n_live = live ? *live_n : N;
    const bool listed = live != nullptr && n_live < N - (N >> 2);
    const uint32_t n_scan = listed ? n_live : N;
    // A short list does not need all of a slice's chunks: an item costs ~10 us of zeroing / flushing / barriers
    // whatever it scans (measured: with 95 % of the samples dead the launch only got 15 % faster), so only as many
    // chunks stay active as have a full pass (list_pass = 4096 samples) to scan; the others leave at once.  The slice of
    // a chunked item is flushed with atomics into a pre-zeroed range, which any number of active chunks satisfies.
    // (list_pass = 1024, a stream layout's coarse levels behind k_live_rows: EVERY listed sample carries a gradient there
    // and it is their visits that cost, not the scan -- 31 K listed samples on 7 of a slice's 28 chunks took 25 us where the
    // full scan of 1.5 M mostly dead ones on all 28 takes 12.)
    uint32_t n_act = n_chunks;
    if (listed && n_chunks > 1u) {
        n_act = max(1u, min(n_chunks, n_scan / list_pass));
        if (chunk >= n_act) return;
    }

    // The item's sample range is handed out to the WAVES in blocks of 64 x 8 (or 64 x 4) consecutive samples from a
    // counter in LDS: with a fixed stride per wave the waves whose samples happen to hit this slice finish last and the
    // other fifteen wait at the barrier -- 20-25 % of an item's cycles by the phase clocks.
    __shared__ uint32_t s_next;
    GP_CLK(go0);
    if (threadIdx.x == 0) s_next = 0u;
    for (uint32_t e = threadIdx.x; e < 2 * count; e += kLdsBwdBlock) acc[e] = (typename ACC::T)0;
    __syncthreads();
    GP_CLK(go1);
    const uint32_t lane_id = threadIdx.x & 63u;
    auto wave_grab = [&](uint32_t n) -> uint32_t {
        uint32_t c = 0u;
        if (lane_id == 0u) c = atomicAdd(&s_next, n);
        return (uint32_t)__builtin_amdgcn_readfirstlane((int)c);
    };

    // (chunk boundaries on multiples of 8 samples: the run-merging scan loads 8 consecutive samples per lane)
    const uint32_t per_chunk = ((n_scan + n_act - 1) / n_act + 7u) & ~7u;
    const uint32_t begin = min(n_scan, chunk * per_chunk);
    const uint32_t end = min(n_scan, begin + per_chunk);
    // Samples are taken kUnroll at a time per thread with all of their loads issued up front: the
    // loop is otherwise one dependent L2 round trip per sample.
    constexpr uint32_t kUnroll = 4;
    const uint32_t mask = size - 1u;
    const uint32_t res2 = res * res;
    // (hashed levels) both x corners of a (y, z) pair share a slice when the slice size is a power of two
    // that exceeds every x coordinate
    const bool pair_bins = hashed && (ACC::kEntries & (ACC::kEntries - 1u)) == 0u && res + 1u < ACC::kEntries &&
                           (first & (ACC::kEntries - 1u)) == 0u && count == ACC::kEntries;
    // Integer accumulators cannot carry inf / NaN: a non-finite dy (fp16 overflow of the scaled loss gradient) is
    // remembered here and poisons the slice's first gradient entry after the flush, so that the optimiser's
    // non-finite check sees it exactly as it would with floating-point accumulation.
    bool bad = false;
    if (merge && !hashed) {
        // Run-merging scan of a DENSE level (option grid_bwd_runs).  Consecutive samples are neighbours on a ray and a
        // coarse cell holds a run of them: a lane takes 8 CONSECUTIVE samples (a wave 512, all 8 loads in flight at
        // once), sums the 8 x 2 corner contributions of the current cell in fp32 registers and goes to the LDS
        // accumulators once per run -- index arithmetic, slice tests, float -> fixed conversions and atomics per RUN
        // instead of per sample, and the lanes of one atomic instruction are 8 samples apart instead of adjacent
        // (the per-sample form had 2/3 of its LDS cycles in same-address conflicts).  A run whose 8 corners all
        // miss the slice costs the cell computation only.
        constexpr uint32_t kRun = 8;
        float a0[8], a1[8];
        uint32_t cx = 0, cy = 0, cz = 0, cbase = 0;
        bool open = false, hit = false;
        const uint32_t span = 1u + res + res2;  // largest corner offset from the cell's base index
        auto flush = [&]() {
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) {
                uint32_t i0 = cbase + ((j & 1u) ? res : 0u) + ((j & 2u) ? res2 : 0u);
                uint32_t i1 = i0 + 1u;
                if (i1 >= size) {
                    i0 %= size;
                    i1 %= size;
                }
                const uint32_t r0 = i0 - first, r1 = i1 - first;  // unsigned wrap -> huge when below the slice
                if (r0 < count) ACC::add(acc, r0, a0[2 * j], a1[2 * j], sc);
                if (r1 < count) ACC::add(acc, r1, a0[2 * j + 1], a1[2 * j + 1], sc);
            }
        };
        auto visit = [&](float px, float py, float pz, float2 d) {
            bad = bad || !(fabsf(d.x) < INFINITY) || !(fabsf(d.y) < INFINITY);
            if (d.x == 0.f && d.y == 0.f) return;
            const Corner c = grid_cell(scale, px, py, pz);
            if (!open || c.px != cx || c.py != cy || c.pz != cz) {
                if (open && hit) flush();
                cx = c.px;
                cy = c.py;
                cz = c.pz;
                open = true;
                cbase = c.px + c.py * res + c.pz * res2;
                // corners lie in [cbase, cbase + span] (or wrap, upper domain face only: treated as a hit)
                hit = cbase + span >= size || (cbase + span >= first && cbase < first + count);
                if (hit) {
#pragma unroll
                    for (int k = 0; k < 8; ++k) a0[k] = a1[k] = 0.f;
                }
            }
            if (!hit) return;
            const float wx0 = 1.f - c.wx, wy0 = 1.f - c.wy, wz0 = 1.f - c.wz;
            const float wyz[4] = {wy0 * wz0, c.wy * wz0, wy0 * c.wz, c.wy * c.wz};
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) {
                const float w0 = wx0 * wyz[j], w1 = c.wx * wyz[j];
                a0[2 * j] += w0 * d.x;
                a1[2 * j] += w0 * d.y;
                a0[2 * j + 1] += w1 * d.x;
                a1[2 * j + 1] += w1 * d.y;
            }
        };
        bool vec = false;
        if constexpr (SOA && sizeof(DY2) == 4) {
            vec = !listed && (N & 3u) == 0u && (((uintptr_t)dy) & 15u) == 0u && (((uintptr_t)x) & 15u) == 0u;
        }
        // (a list of samples that ALL carry a gradient -- list_pass < 4096, k_live_rows on a trained field, one sample per
        // ray: a lane takes ONE sample of a 64-sample block; list neighbours are not neighbours in space, there is nothing
        // to merge, and a short list then reaches every wave: 1.1 K samples per item are 17 blocks of 64 but only 3 of 512)
        const bool single = listed && list_pass < 4096u;
        const uint32_t kGrab = single ? 64u : 64u * kRun;
        const uint32_t kLaneRun = single ? 1u : kRun;
        for (uint32_t c0 = wave_grab(kGrab); begin + c0 < end; c0 = wave_grab(kGrab)) {
            const uint32_t b0 = begin + c0 + lane_id * kLaneRun;
            if (b0 >= end) continue;
            open = false;
            hit = false;
            bool done = false;
            if constexpr (SOA && sizeof(DY2) == 4) {
                if (vec && b0 + kRun <= end) {
                    const float4* __restrict__ xp = reinterpret_cast<const float4*>(x + 3 * (size_t)b0);
                    const uint4* __restrict__ dp = reinterpret_cast<const uint4*>(dy + (size_t)level * N + b0);
                    const float4 p0 = xp[0], p1 = xp[1], p2 = xp[2], p3 = xp[3], p4 = xp[4], p5 = xp[5];
                    const uint4 q0 = dp[0], q1 = dp[1];
                    visit(p0.x, p0.y, p0.z, dy2f(__builtin_bit_cast(DY2, q0.x)));
                    visit(p0.w, p1.x, p1.y, dy2f(__builtin_bit_cast(DY2, q0.y)));
                    visit(p1.z, p1.w, p2.x, dy2f(__builtin_bit_cast(DY2, q0.z)));
                    visit(p2.y, p2.z, p2.w, dy2f(__builtin_bit_cast(DY2, q0.w)));
                    visit(p3.x, p3.y, p3.z, dy2f(__builtin_bit_cast(DY2, q1.x)));
                    visit(p3.w, p4.x, p4.y, dy2f(__builtin_bit_cast(DY2, q1.y)));
                    visit(p4.z, p4.w, p5.x, dy2f(__builtin_bit_cast(DY2, q1.z)));
                    visit(p5.y, p5.z, p5.w, dy2f(__builtin_bit_cast(DY2, q1.w)));
                    done = true;
                }
            }
            if (!done && single) {
                const uint32_t id = live[b0];
                const DY2 dd = SOA ? dy[(size_t)level * N + id] : dy[(size_t)id * g.n_levels + level];
                visit(x[3 * (size_t)id + 0], x[3 * (size_t)id + 1], x[3 * (size_t)id + 2], dy2f(dd));
                done = true;
            }
            if (!done) {
                const uint32_t stop = min(end, b0 + kRun);
                for (uint32_t j = b0; j < stop; ++j) {
                    const uint32_t i = listed ? live[j] : j;
                    const DY2 d2 = SOA ? dy[(size_t)level * N + i] : dy[(size_t)i * g.n_levels + level];
                    visit(x[3 * (size_t)i + 0], x[3 * (size_t)i + 1], x[3 * (size_t)i + 2], dy2f(d2));
                }
            }
            if (open && hit) flush();
        }
    } else if (pair_bins && ring_off != 0u) {
        // HASHED level with a hit queue (kHitCap).  Everything up to the slice test runs for all 64 lanes; the pairs that
        // fall into this slice (one in `slices of the level` on average) are pushed into the wave's ring -- 16 bytes:
        // in-slice offset | px << 14, w_y w_z dy_0, w_y w_z dy_1, w_x -- and whenever 64 are waiting the whole wave
        // splits them into their two x corners and adds them.  The ring is private to the wave (LDS operations of one
        // wave execute in order: no barrier), head and fill level are wave-uniform scalars, and every push sits in
        // wave-uniform control flow (a ballot under a lane-divergent branch would let the lanes disagree about them).
        uint4* const ring = reinterpret_cast<uint4*>(reinterpret_cast<unsigned char*>(lds_raw) + ring_off) +
                            (threadIdx.x >> 6) * kHitCap;
        uint32_t q_head = 0u, q_fill = 0u;
        auto q_drain = [&](uint32_t n) {  // the n <= 64 oldest entries
            if (lane_id < n) {
                uint32_t p = q_head + lane_id;
                if (p >= kHitCap) p -= kHitCap;
                const uint4 e = ring[p];
                const uint32_t lo = e.x & (ACC::kEntries - 1u), px = e.x >> 14;
                const float u0 = __uint_as_float(e.y), u1 = __uint_as_float(e.z), wx = __uint_as_float(e.w);
                const float wx0 = 1.f - wx;
                ACC::add(acc, lo ^ px, wx0 * u0, wx0 * u1, sc);
                ACC::add(acc, lo ^ (px + 1u), wx * u0, wx * u1, sc);
            }
            q_head += n;
            if (q_head >= kHitCap) q_head -= kHitCap;
            q_fill -= n;
        };
        auto q_push = [&](bool hit, uint32_t word, float u0, float u1, float wx) {
            const unsigned long long m = __ballot(hit);
            const uint32_t c = (uint32_t)__popcll(m);
            if (q_fill + c > kHitCap) {  // (cannot happen below 64 waiting entries unless > 63 lanes hit at once)
                while (q_fill) q_drain(min(q_fill, 64u));
            }
            if (hit) {
                uint32_t p = q_head + q_fill + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                if (p >= kHitCap) p -= kHitCap;
                ring[p] = make_uint4(word, __float_as_uint(u0), __float_as_uint(u1), __float_as_uint(wx));
            }
            q_fill += c;
            if (q_fill >= 64u) q_drain(64u);
        };
        for (uint32_t c0 = wave_grab(64u * kUnroll); begin + c0 < end; c0 = wave_grab(64u * kUnroll)) {
            const uint32_t i0 = begin + c0 + lane_id;
            float2 dv[kUnroll];
            float xv[kUnroll][3];
            uint32_t sid[kUnroll];
#pragma unroll
            for (uint32_t u = 0; u < kUnroll; ++u) {
                const uint32_t j = i0 + u * 64u;
                sid[u] = j < end ? (listed ? live[j] : j) : 0u;
            }
#pragma unroll
            for (uint32_t u = 0; u < kUnroll; ++u) {
                const uint32_t i = sid[u];
                dv[u] = make_float2(0.f, 0.f);
                xv[u][0] = xv[u][1] = xv[u][2] = 0.f;
                if (i0 + u * 64u < end) {
                    const DY2 d2 = SOA ? dy[(size_t)level * N + i] : dy[(size_t)i * g.n_levels + level];
                    dv[u] = dy2f(d2);
                    xv[u][0] = x[3 * (size_t)i + 0];
                    xv[u][1] = x[3 * (size_t)i + 1];
                    xv[u][2] = x[3 * (size_t)i + 2];
                }
            }
#pragma unroll
            for (uint32_t u = 0; u < kUnroll; ++u) {
                const float2 d = dv[u];
                bad = bad || !(fabsf(d.x) < INFINITY) || !(fabsf(d.y) < INFINITY);
                const bool lv = d.x != 0.f || d.y != 0.f;  // (out-of-range slots carry d = 0)
                const Corner c = grid_cell(scale, xv[u][0], xv[u][1], xv[u][2]);
                const float wy0 = 1.f - c.wy, wz0 = 1.f - c.wz;
                const float wyz[4] = {wy0 * wz0, c.wy * wz0, wy0 * c.wz, c.wy * c.wz};
                const uint32_t hy0 = c.py * 2654435761u, hy1 = hy0 + 2654435761u;
                const uint32_t hz0 = c.pz * 805459861u, hz1 = hz0 + 805459861u;
                const uint32_t a[4] = {hy0 ^ hz0, hy1 ^ hz0, hy0 ^ hz1, hy1 ^ hz1};
#pragma unroll
                for (uint32_t j = 0; j < 4; ++j) {
                    const uint32_t h = a[j] & mask;
                    q_push(lv && (h & ~(ACC::kEntries - 1u)) == first, (h & (ACC::kEntries - 1u)) | (c.px << 14),
                           wyz[j] * d.x, wyz[j] * d.y, c.wx);
                }
            }
        }
        while (q_fill) q_drain(min(q_fill, 64u));
    } else
    for (uint32_t c0 = wave_grab(64u * kUnroll); begin + c0 < end; c0 = wave_grab(64u * kUnroll)) {
        const uint32_t i0 = begin + c0 + lane_id;
        float2 dv[kUnroll];
        float xv[kUnroll][3];
        uint32_t sid[kUnroll];
#pragma unroll
        for (uint32_t u = 0; u < kUnroll; ++u) {  // (one extra round trip per pass when the list is used)
            const uint32_t j = i0 + u * 64u;
            sid[u] = j < end ? (listed ? live[j] : j) : 0u;
        }
#pragma unroll
        for (uint32_t u = 0; u < kUnroll; ++u) {
            const uint32_t i = sid[u];
            dv[u] = make_float2(0.f, 0.f);
            xv[u][0] = xv[u][1] = xv[u][2] = 0.f;
            if (i0 + u * 64u < end) {
                const DY2 d2 = SOA ? dy[(size_t)level * N + i] : dy[(size_t)i * g.n_levels + level];
                dv[u] = dy2f(d2);
                xv[u][0] = x[3 * (size_t)i + 0];
                xv[u][1] = x[3 * (size_t)i + 1];
                xv[u][2] = x[3 * (size_t)i + 2];
            }
        }
#pragma unroll
        for (uint32_t u = 0; u < kUnroll; ++u) {
            const float2 d = dv[u];
            bad = bad || !(fabsf(d.x) < INFINITY) || !(fabsf(d.y) < INFINITY);
            if (d.x == 0.f && d.y == 0.f) continue;
            const Corner c = grid_cell(scale, xv[u][0], xv[u][1], xv[u][2]);
            const float wx0 = 1.f - c.wx, wy0 = 1.f - c.wy, wz0 = 1.f - c.wz;
            const float wyz[4] = {wy0 * wz0, c.wy * wz0, wy0 * c.wz, c.wy * c.wz};
            if (hashed) {
                // two integer multiplies per sample; the 4 (y, z) corner pairs are xor combinations
                const uint32_t hy0 = c.py * 2654435761u, hy1 = hy0 + 2654435761u;
                const uint32_t hz0 = c.pz * 805459861u, hz1 = hz0 + 805459861u;
                const uint32_t a[4] = {hy0 ^ hz0, hy1 ^ hz0, hy0 ^ hz1, hy1 ^ hz1};
                if (pair_bins) {
                    // power-of-two slices and px + 1 < slice size: the x coordinate only touches index bits
                    // below the slice bits, so both x corners of a (y, z) pair are in the SAME slice and one
                    // test on the (y, z) hash decides both
#pragma unroll
                    for (uint32_t j = 0; j < 4; ++j) {
                        const uint32_t h = a[j] & mask;
                        if ((h & ~(ACC::kEntries - 1u)) == first) {
                            const float wj = wyz[j];
                            const uint32_t lo = h & (ACC::kEntries - 1u);
                            ACC::add(acc, lo ^ c.px, wx0 * wj * d.x, wx0 * wj * d.y, sc);
                            ACC::add(acc, lo ^ (c.px + 1u), c.wx * wj * d.x, c.wx * wj * d.y, sc);
                        }
                    }
                } else {
#pragma unroll
                    for (uint32_t j = 0; j < 4; ++j) {
                        const uint32_t r0 = ((c.px ^ a[j]) & mask) - first, r1 = (((c.px + 1u) ^ a[j]) & mask) - first;
                        const float wj = wyz[j];
                        if (r0 < count) ACC::add(acc, r0, wx0 * wj * d.x, wx0 * wj * d.y, sc);
                        if (r1 < count) ACC::add(acc, r1, c.wx * wj * d.x, c.wx * wj * d.y, sc);
                    }
                }
            } else {
                // dense stride index: one base + adds; the wrap (positions on the upper domain face only) sits
                // behind a branch that is almost never taken
                const uint32_t base = c.px + c.py * res + c.pz * res2;
#pragma unroll
                for (uint32_t j = 0; j < 4; ++j) {
                    uint32_t i0 = base + ((j & 1u) ? res : 0u) + ((j & 2u) ? res2 : 0u);
                    uint32_t i1 = i0 + 1u;
                    if (i1 >= size) {
                        i0 %= size;
                        i1 %= size;
                    }
                    const uint32_t r0 = i0 - first, r1 = i1 - first;  // unsigned wrap -> huge when below the slice
                    const float wj = wyz[j];
                    if (r0 < count) ACC::add(acc, r0, wx0 * wj * d.x, wx0 * wj * d.y, sc);
                    if (r1 < count) ACC::add(acc, r1, c.wx * wj * d.x, c.wx * wj * d.y, sc);
                }
            }
        }
    }
    GP_CLK(go2);
    __syncthreads();
    GP_CLK(go3);
    float* __restrict__ gr = grad + 2 * ((size_t)off + first);
    if (n_chunks == 1) {
        for (uint32_t e = threadIdx.x; e < 2 * count; e += kLdsBwdBlock) gr[e] = ACC::get(acc, e, sc);
    } else {
        for (uint32_t e = threadIdx.x; e < 2 * count; e += kLdsBwdBlock) {
            const float v = ACC::get(acc, e, sc);
            if (v != 0.f) atomicAdd(gr + e, v);
        }
    }
    // (no LDS to spare for a block-wide vote: one atomic per affected wave, after every plain store has retired)
    __syncthreads();
#ifdef NVO_GRID_PHASE
    if (threadIdx.x == 0) {
        GP_CLK(go4);
        const int o = hashed ? 24 : 16;
        GP_ADD(o + 0, go1 - go0); GP_ADD(o + 1, go2 - go1); GP_ADD(o + 2, go3 - go2); GP_ADD(o + 3, go4 - go3); GP_ADD(o + 4, 1);
        if (level < 5u) { GP_ADD(38 + level, go2 - go1); GP_ADD(43 + level, 1); }  // scan cycles / items per level (L <= 5 grids)
    }
#endif
    if (__ballot(bad) != 0ull && (threadIdx.x & 63u) == 0u) {
        atomicAdd(gr, __builtin_nanf(""));
        if (nf_flag) atomicOr(nf_flag, 1u);  // (the optimiser's overflow flag, raised at the source)
    }
}

template <bool SOA, typename DY2>
__global__ void __launch_bounds__(kLdsBwdBlock)
k_grid_bwd_lds_legacy(NvoGridLevels g, uint32_t N, const float* __restrict__ x,
               const DY2* __restrict__ dy, float* __restrict__ grad,
               const uint4* __restrict__ items, const unsigned long long* __restrict__ l1,
               const uint32_t* __restrict__ live, uint32_t* __restrict__ nf_flag, const uint32_t* __restrict__ live_n,
               uint32_t ring_off, const float* __restrict__ ext_l1, uint32_t ext_blocks, uint32_t ext_stride,
               uint32_t list_pass) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const uint4 item = items[blockIdx.x];  // {level, first entry, chunk, n_chunks | accumulator-kind flags}
    const uint32_t n_chunks = item.w & 0x1FFFFFFFu;
    const bool merge = (item.w >> 29) & 1u;
    const uint32_t level = item.x & 0xFFu, cap = item.x >> 8;  // cap: entries per slice of this level
    // 32-bit accumulators, L1 norms delivered by the fused-MLP backward that wrote dy (NvoGridSlices::ext_l1): the
    // workgroups' partial sums are added up in a fixed order (same scale in every item and every run)
    __shared__ float s_l1[kLdsBwdBlock / 64][2];
    float l1e[2] = {0.f, 0.f};
    if (ext_l1 && ((item.w >> 30) & 1u) && !(item.w >> 31)) {
        float a = 0.f, b = 0.f;
        for (uint32_t blk = threadIdx.x; blk < ext_blocks; blk += kLdsBwdBlock) {
            a += ext_l1[(size_t)blk * ext_stride + 2 * level];
            b += ext_l1[(size_t)blk * ext_stride + 2 * level + 1];
        }
        a = nvo_wave_sum(a);
        b = nvo_wave_sum(b);
        if ((threadIdx.x & 63u) == 0u) {
            s_l1[threadIdx.x >> 6][0] = a;
            s_l1[threadIdx.x >> 6][1] = b;
        }
        __syncthreads();
#pragma unroll
        for (int w = 0; w < kLdsBwdBlock / 64; ++w) {
            l1e[0] += s_l1[w][0];
            l1e[1] += s_l1[w][1];
        }
        // upper bound of the exact sum (fp32 summation error of <= a few thousand terms) -- the 2^29 scale leaves a
        // factor of four of headroom inside int32 on top of this
        l1e[0] = l1e[0] * 1.001f + 1e-30f;
        l1e[1] = l1e[1] * 1.001f + 1e-30f;
    }
    if (item.w >> 31) {
        grid_bwd_item_legacy<AccFloat, SOA, DY2>(g, N, x, dy, grad, level, item.y, item.z, n_chunks, lds_raw,
                                          AccScale{0.f, 0.f, 0.f, 0.f}, live, merge, cap, nf_flag, live_n, 0u, list_pass);
    } else if ((item.w >> 30) & 1u) {
        const float l1x = ext_l1 ? l1e[0] : (float)l1[2 * level] * (1.f / 256.f);
        const float l1y = ext_l1 ? l1e[1] : (float)l1[2 * level + 1] * (1.f / 256.f);
        AccScale sc;
        sc.s0 = l1x > 0.f ? 536870912.f / l1x : 0.f;  // 2^29 / L1
        sc.s1 = l1y > 0.f ? 536870912.f / l1y : 0.f;
        sc.inv0 = l1x * (1.f / 536870912.f);
        sc.inv1 = l1y * (1.f / 536870912.f);
        grid_bwd_item_legacy<AccFixed32, SOA, DY2>(g, N, x, dy, grad, level, item.y, item.z, n_chunks, lds_raw, sc, live,
                                            merge, cap, nf_flag, live_n, ring_off, list_pass);
    } else {
        grid_bwd_item_legacy<AccFixed, SOA, DY2>(g, N, x, dy, grad, level, item.y, item.z, n_chunks, lds_raw,
                                          AccScale{0.f, 0.f, 0.f, 0.f}, live, merge, cap, nf_flag, live_n, 0u, list_pass);
    }
}

}  // namespace

int nvo_grid_bwd_lds_legacy_launch(const NvoGridLevels& g, const NvoGridSlices* slices, hipStream_t stream, uint32_t N,
                                   const float* x, const void* dy, int dy_fmt, bool soa, float* grad, size_t lds,
                                   uint32_t ring_off, const uint32_t* live) {
    const dim3 grid(slices->n_slices), block(kLdsBwdBlock);
#define NVO_LAUNCH_LDS(SOA_, T_)                                                              \
    do {                                                                                      \
        static bool attr_set = false; /* >64 KiB of dynamic LDS needs an explicit opt-in */   \
        if (!attr_set) {                                                                      \
            NVO_CHECK_HIP(hipFuncSetAttribute((const void*)k_grid_bwd_lds_legacy<SOA_, T_>,   \
                                              hipFuncAttributeMaxDynamicSharedMemorySize,     \
                                              (int)kLdsBwdBytes - 256)); /* (static: work counter) */ \
            attr_set = true;                                                                  \
        }                                                                                     \
        NVO_LAUNCH((k_grid_bwd_lds_legacy<SOA_, T_>), grid, block, lds, stream, g, N, x,      \
                   (const T_*)dy, grad, (const uint4*)slices->d_level, slices->d_l1, live, slices->nf_flag, \
                   slices->d_live_n, ring_off, slices->ext_l1, slices->ext_blocks, slices->ext_l1_stride,   \
                   slices->ext_list ? 1024u : 4096u);                                         \
    } while (0)
#define NVO_LAUNCH_LDS_DY(SOA_)                                    \
    do {                                                           \
        if (dy_fmt == NVO_DY_FLOAT) NVO_LAUNCH_LDS(SOA_, float2);  \
        else if (dy_fmt == NVO_DY_BF16) NVO_LAUNCH_LDS(SOA_, Bf2); \
        else NVO_LAUNCH_LDS(SOA_, __half2);                        \
    } while (0)
    if (soa) NVO_LAUNCH_LDS_DY(true); else NVO_LAUNCH_LDS_DY(false);
#undef NVO_LAUNCH_LDS_DY
#undef NVO_LAUNCH_LDS
    NVO_CHECK_LAUNCH();
    return NVO_OK;
}
