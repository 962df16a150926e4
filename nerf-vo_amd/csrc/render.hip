// Per-ray kernels of the mapping training step for gfx950, ONE WAVE (64 lanes) PER RAY:
//   k_weights_pdf      density activation (trunc_exp) + volume-rendering weights + (optionally)
//                      histogram-CDF resampling of the next level's bins (PDFSampler)
//   k_main_render_loss compositing (rgb with last-sample background, accumulation, median and
//                      expected depth) fused with the rgb / distortion / depth losses and their
//                      gradients w.r.t. per-sample colour and density pre-activation
//   k_prop_loss        interlevel (mip-NeRF 360 outer-measure) + depth loss of one proposal level and
//                      the gradient w.r.t. that level's density pre-activation
// Prefix / suffix sums over a ray's samples are wavefront scans (shuffle network) with a carry
// across 64-sample chunks; per-ray scratch lives in the wave's private LDS slice.
// Replaces nerfstudio's torch-op chains RaySamples.get_weights, PDFSampler, RGBRenderer /
// AccumulationRenderer / DepthRenderer, interlevel_loss / distortion_loss / ds_nerf_depth_loss
// (reference hooks /root/reference/nerf_vo/mapping/
// nerfstudio_utils.py:337-350 and nerfstudio.py:71-82 for the loss multipliers).
// CPU restatement: oracle/rays.py.
#include "nvo_kernels.h"
#include "../../include/nerfvo_hip.h"

#include <float.h>

namespace {

constexpr int kRayBlock = 256;          // 4 waves = 4 rays per workgroup
constexpr int kRaysPerBlock = kRayBlock / 64;
constexpr int kMaxS = 256;              // samples per ray handled by the LDS scratch
constexpr int kChunks = kMaxS / 64;     // 64-sample chunks of the longest ray
constexpr float kLossEps = 1.0e-7f;     // nerfstudio losses.EPS

// (DPP forms, nvo_common.h: the shuffle forms were six dependent LDS round trips each)
__device__ __forceinline__ float wave_incl_scan(float v, int) { return nvo_wave_incl_scan(v); }
__device__ __forceinline__ float wave_sum(float v) { return nvo_wave_sum(v); }

__device__ __forceinline__ float nan_to_num(float v) {
    if (isnan(v)) return 0.f;
    if (isinf(v)) return v > 0.f ? FLT_MAX : -FLT_MAX;
    return v;
}

__device__ __forceinline__ float spacing_fn(float x) { return x < 1.f ? x * 0.5f : 1.f - 1.f / (2.f * x); }
__device__ __forceinline__ float spacing_fn_inv(float x) { return x < 0.5f ? 2.f * x : 1.f / (2.f - 2.f * x); }

// first index in a[0..n) with a[idx] > v   (torch.searchsorted(..., side="right"))
__device__ __forceinline__ int upper_bound(const float* a, int n, float v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] > v) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// Per-ray forward quantities from the density pre-activation; fills LDS arrays w[] and Tr[].
// sigma = selector * exp(pre + bias); w_i = (1 - exp(-delta_i sigma_i)) * exp(-sum_{j<i} delta_j sigma_j)
__device__ __forceinline__ void ray_weights(int lane, uint32_t S, const nvo_h16* __restrict__ pre, bool bf,
                                            uint32_t pre_stride, const float* __restrict__ x01,
                                            const float* __restrict__ tb, float bias,
                                            float* __restrict__ sigma_out, float* w, float* Tr) {
    float carry = 0.f;
    // One wave walks the ray in chunks of 64 samples with a carry between them: the NEXT chunk's inputs are requested
    // (unconditionally, at a clamped index: a load behind a divergent branch makes the join wait for everything in
    // flight) before the current chunk is scanned, so a 256-sample ray pays one memory round trip instead of four.
    struct In { float x0, pr, t0, t1; };
    auto fetch = [&](uint32_t base) {
        const uint32_t i = min(base + (uint32_t)lane, S - 1u);
        In v;
        v.x0 = x01[3 * (size_t)i];
        v.pr = nvo_ld16(pre + (size_t)i * pre_stride, bf);
        v.t0 = tb[i];
        v.t1 = tb[i + 1];
        return v;
    };
    In cur = fetch(0);
    for (uint32_t base = 0; base < S; base += 64) {
        const uint32_t i = base + lane;
        In nxt = cur;
        if (base + 64 < S) nxt = fetch(base + 64);  // (wave-uniform; single-chunk rays request nothing twice)
        float dd = 0.f, sg = 0.f;
        if (i < S) {
            const bool sel = cur.x0 > 0.f;
            // (exponent capped at 60: sigma <= 1.1e26 -- alpha is 1 to the last bit long before that -- so that a run whose
            // density pre-activations have blown up cannot put inf - inf = NaN into the transmittance and, through it, a
            // NaN that no loss scale can back off from into every gradient of the step; trunc_exp's forward is exp(x))
            sg = sel ? __expf(fminf(cur.pr + bias, 60.f)) : 0.f;
            dd = (cur.t1 - cur.t0) * sg;
            if (sigma_out) sigma_out[i] = sg;
        }
        cur = nxt;
        const float incl = wave_incl_scan(dd, lane) + carry;
        const float T = __expf(-(incl - dd));
        if (i < S) {
            w[i] = nan_to_num((1.f - __expf(-dd)) * T);
            Tr[i] = T;
        }
        carry = nvo_wave_bcast(incl, 63);
    }
}

// ---- forward and backward one 64-sample chunk at a time, on operands the caller has loaded at the kernel entry -----
// (k_main_render_loss, k_prop_loss)  A launch of these kernels is ONE round of waves (a ray each), so it lasts as long as
// a ray's dependent chain: every global load of the ray is requested before the first wait and consumed later, and the
// backward takes the selector, pre + bias and the interval length from the forward's registers instead of loading them
// again.  The forward is ray_weights' arithmetic expression by expression (the library is built with -ffp-contract=off).
// k_weights_pdf keeps the whole-ray form above: with its loads up front it measured no faster (EXPERIMENTS.md 12.4).
// a lane's inputs of one chunk, requested at index min(base + lane, S - 1); pr stays in its 16-bit format until it is used
// (a conversion next to the load waits for it, and the requests behind it would queue up after that wait)
struct RayIn { float x0; nvo_h16 pr; float t0, t1; };
__device__ __forceinline__ float h16_to_float(nvo_h16 raw, bool bf) {  // (nvo_ld16 without the load)
    return bf ? __uint_as_float((uint32_t)raw << 16) : (float)__builtin_bit_cast(_Float16, raw);
}
__device__ __forceinline__ RayIn ray_fetch(int lane, uint32_t S, uint32_t base, const nvo_h16* __restrict__ pre, bool bf,
                                           uint32_t pre_stride, const float* __restrict__ x01,
                                           const float* __restrict__ tb) {
    const uint32_t i = min(base + (uint32_t)lane, S - 1u);
    RayIn v;
    v.x0 = x01[3 * (size_t)i];
    v.pr = pre[(size_t)i * pre_stride];
    v.t0 = tb[i];
    v.t1 = tb[i + 1];
    return v;
}
// Everything requested above this line stays above it and nothing below it moves up: the loads of a kernel's entry are
// not sunk to their first use (no instruction; the registers are not named, so nothing waits here).
__device__ __forceinline__ void loads_issued() { asm volatile("" ::: "memory"); }

struct RayKeep { bool sel; float x, delta; };  // what the backward needs again: selector, pre + bias, t[i+1] - t[i]
// forward of one chunk; valid = the lane's sample exists (a lane without one holds the last sample's inputs: selected
// away, never multiplied in).  w = 0 on such a lane.
__device__ __forceinline__ void ray_weights_chunk(int lane, const RayIn& in, bool bf, bool valid, float bias, float& carry,
                                                  float& w, float& T, RayKeep& k) {
    k.sel = in.x0 > 0.f;
    k.x = h16_to_float(in.pr, bf) + bias;
    k.delta = in.t1 - in.t0;
    float dd = 0.f, sg = 0.f;
    if (valid) {
        sg = k.sel ? __expf(fminf(k.x, 60.f)) : 0.f;  // (the cap: see ray_weights)
        dd = k.delta * sg;
    }
    const float incl = wave_incl_scan(dd, lane) + carry;
    T = __expf(-(incl - dd));
    w = valid ? nan_to_num((1.f - __expf(-dd)) * T) : 0.f;
    carry = nvo_wave_bcast(incl, 63);
}
// backward of one chunk: g = dL/dw of the lane's sample, total = sum over the ray of g_i w_i, carry = that sum over the
// chunks before this one; returns dL/dpre * loss_scale in the 16-bit format it is stored in
// dL/dsigma_k = delta_k [ g_k (T_k - w_k) - sum_{i>k} g_i w_i ],  dsigma/dpre = exp(clamp(pre+bias,-15,15))
// overflow (per lane, OR-ed in): a gradient of this ray does not survive that format
__device__ __forceinline__ nvo_h16 ray_weights_bwd_chunk(int lane, bool valid, const RayKeep& k, float g, float w, float T,
                                                         float total, float& carry, float loss_scale, bool bf,
                                                         bool& overflow) {
    const float fmt_max = bf ? 3.0e38f : 65504.0f;
    const float gw = valid ? g * w : 0.f;
    const float incl = wave_incl_scan(gw, lane) + carry;
    float d = 0.f;
    if (valid && k.sel) {
        const float dsig = k.delta * (g * (T - w) - (total - incl));
        d = dsig * __expf(fminf(fmaxf(k.x, -15.f), 15.f));
    }
    if (valid) overflow = overflow || !(fabsf(d * loss_scale) <= fmt_max);
    carry = nvo_wave_bcast(incl, 63);
    return nvo_cvt16(d * loss_scale, bf);
}
// ------------------------------------------------------------------------------------------------
// weights (+ PDF resampling)
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kRayBlock)
k_weights_pdf(nvo_weights_pdf_args a) {
    __shared__ float lds[kRaysPerBlock][3][kMaxS + 4];
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    const uint32_t r = blockIdx.x * kRaysPerBlock + wib;
    if (r >= a.R) return;
    float* w = lds[wib][0];
    float* Tr = lds[wib][1];
    float* cdf = lds[wib][2];
    const uint32_t S = a.S;
    const size_t so = (size_t)r * S;
    const float* tb = a.tbins + (size_t)r * (S + 1);
    ray_weights(lane, S, (const nvo_h16*)a.pre + so * a.pre_stride, a.act_bf16 != 0, a.pre_stride, a.x01 + 3 * so, tb, a.density_bias,
                a.sigma ? a.sigma + so : nullptr, w, Tr);
    for (uint32_t i = lane; i < S; i += 64) a.weights[so + i] = w[i];
    if (a.S_out == 0) return;

    // ---- PDFSampler: annealed weights -> padded pdf -> clamped cdf (cdf[0] = 0)
    const float anneal = a.anneal_dev ? *a.anneal_dev : a.anneal;
    float part = 0.f;
    for (uint32_t i = lane; i < S; i += 64) {
        const float wa = (anneal == 1.0f ? w[i] : powf(w[i], anneal)) + a.histogram_padding;
        Tr[i] = wa;  // reuse as pdf numerator
        part += wa;
    }
    float sum = wave_sum(part);
    const float padding = fmaxf(1e-5f - sum, 0.f);
    sum += padding;
    const float pad_each = padding / (float)S;
    float carry = 0.f;
    for (uint32_t base = 0; base < S; base += 64) {
        const uint32_t i = base + lane;
        const float p = (i < S) ? (Tr[i] + pad_each) / sum : 0.f;
        const float incl = wave_incl_scan(p, lane) + carry;
        if (i < S) cdf[i + 1] = fminf(1.f, incl);
        carry = nvo_wave_bcast(incl, 63);
    }
    if (lane == 0) cdf[0] = 0.f;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

    const float* sb = a.sbins + (size_t)r * (S + 1);
    const uint32_t nb = a.S_out + 1;
    const float inv_nb = 1.0f / (float)nb;
    const float shift = a.jitter ? a.jitter[r] * inv_nb : 0.5f * inv_nb;
    const float s_near = spacing_fn(a.near_plane), s_far = spacing_fn(a.far_plane);
    for (uint32_t j = lane; j < nb; j += 64) {
        const float u = (float)j * inv_nb + shift;
        const int inds = upper_bound(cdf, (int)S + 1, u);
        const int below = min(max(inds - 1, 0), (int)S), above = min(max(inds, 0), (int)S);
        const float c0 = cdf[below], c1 = cdf[above];
        float t = (u - c0) / (c1 - c0);
        if (isnan(t)) t = 0.f;
        t = fminf(fmaxf(t, 0.f), 1.f);
        const float b = sb[below] + t * (sb[above] - sb[below]);
        const float tv = spacing_fn_inv(b * s_far + (1.f - b) * s_near);
        a.sbins_out[(size_t)r * nb + j] = b;
        a.tbins_out[(size_t)r * nb + j] = tv;
        if (a.x01_out) w[j] = tv;  // the weights are in global memory already: reuse their LDS row
    }
    if (a.x01_out) {  // fused nvo_sample_positions of the resampled level
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const float o[3] = {a.origins[3 * (size_t)r], a.origins[3 * (size_t)r + 1], a.origins[3 * (size_t)r + 2]};
        const float d[3] = {a.directions[3 * (size_t)r], a.directions[3 * (size_t)r + 1], a.directions[3 * (size_t)r + 2]};
        for (uint32_t j = lane; j < a.S_out; j += 64) {
            float p[3];
            nvo_contract_position01(o, d, (w[j] + w[j + 1]) * 0.5f, p);
            float* xo = a.x01_out + 3 * ((size_t)r * a.S_out + j);
            xo[0] = p[0]; xo[1] = p[1]; xo[2] = p[2];
        }
    }
}

// ------------------------------------------------------------------------------------------------
// main level: render + losses + gradients
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kRayBlock)
k_main_render_loss(nvo_main_loss_args a) {
    __shared__ float lds[kRaysPerBlock][2][64 + 4];
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    const uint32_t r = blockIdx.x * kRaysPerBlock + wib;
    if (r >= a.R) return;
    float* w = lds[wib][0];   // (read at other lanes' indices by the distortion term only)
    float* ut = lds[wib][1];
    const uint32_t S = a.S;
    const size_t so = (size_t)r * S;
    const float* tb = a.tbins + (size_t)r * (S + 1);
    const float* sb = a.sbins + (size_t)r * (S + 1);
    const nvo_h16* pre = (const nvo_h16*)a.pre + so * a.pre_stride;
    const bool bf = a.act_bf16 != 0;
    const float* x01 = a.x01 + 3 * so;
    const bool act = (uint32_t)lane < S;
    const uint32_t li = min((uint32_t)lane, S - 1u);  // the index every lane loads at: its own sample, or the last one
    // what this call computes (all uniform: tests of arguments); the inference call loads nothing that only training reads
    const bool train = a.dpre != nullptr;
    const bool has_normals = a.dsigma_dx != nullptr;
    const bool use_dist = train && a.distortion_mult != 0.f;
    const bool use_depth = train && a.depth_mult != 0.f && a.gt_depth;
    const bool use_gt_normal = train && has_normals && a.gt_normal && a.normal_mult != 0.f;
    // ---- every global load of the ray, before the first wait
    const RayIn in = ray_fetch(lane, S, 0, pre, bf, a.pre_stride, x01, tb);
    const nvo_h16* cp = (const nvo_h16*)a.rgb + (so + li) * a.rgb_stride;
    const nvo_h16 c16[3] = {cp[0], cp[1], cp[2]};
    float s0 = 0.f, s1 = 0.f;
    if (use_dist) { s0 = sb[li]; s1 = sb[li + 1]; }
    float gd[3] = {0.f, 0.f, 0.f};
    if (has_normals) {
        const float* gp = a.dsigma_dx + 3 * (so + li);
        gd[0] = gp[0]; gd[1] = gp[1]; gd[2] = gp[2];
    }
    float gt[3] = {0.f, 0.f, 0.f}, gtn[3] = {0.f, 0.f, 0.f};
    float gt_z = 0.f, dir_norm = 0.f;
    if (train) {
#pragma unroll
        for (int k = 0; k < 3; ++k) gt[k] = a.gt_rgb[3 * (size_t)r + k];
        if (use_depth) { gt_z = a.gt_depth[r]; dir_norm = a.directions_norm[r]; }
        if (use_gt_normal) {
#pragma unroll
            for (int k = 0; k < 3; ++k) gtn[k] = a.gt_normal[3 * (size_t)r + k];
        }
        if (a.loss_scale_dev) a.loss_scale = *a.loss_scale_dev;  // dynamic loss scale (GradScaler state on the device)
    }
    loads_issued();

    float carry = 0.f, wi, Ti;
    RayKeep keep;
    ray_weights_chunk(lane, in, bf, act, a.density_bias, carry, wi, Ti, keep);
    if (use_dist && act) w[lane] = wi;
    if (a.weights && act) a.weights[so + lane] = wi;

    // ---- composite
    float c[3] = {0.f, 0.f, 0.f};
    if (act) {
        c[0] = h16_to_float(c16[0], bf); c[1] = h16_to_float(c16[1], bf); c[2] = h16_to_float(c16[2], bf);
    }
    const float acc = wave_sum(wi);
    float pix[3], clast[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        clast[k] = nvo_wave_bcast(c[k], (int)S - 1);
        pix[k] = wave_sum(wi * c[k]) + clast[k] * (1.f - acc);
    }
    const float mid = act ? 0.5f * (in.t0 + in.t1) : 0.f;
    // median depth: first sample whose cumulative weight reaches 0.5 (clamped to the last sample)
    const float cum = wave_incl_scan(wi, lane);
    const unsigned long long ballot = __ballot(act && cum >= 0.5f);
    const int med = ballot ? (int)__builtin_ctzll(ballot) : (int)S - 1;
    const float depth_med = nvo_wave_bcast(mid, med);
    if (lane == 0) {
        a.out_rgb[3 * (size_t)r + 0] = pix[0];
        a.out_rgb[3 * (size_t)r + 1] = pix[1];
        a.out_rgb[3 * (size_t)r + 2] = pix[2];
        a.out_depth[r] = depth_med;
        a.out_accumulation[r] = acc;
    }
    if (a.out_expected_depth) {
        const float num = wave_sum(wi * mid);
        if (lane == 0) a.out_expected_depth[r] = num / (acc + 1e-10f);  // clip to [min,max] steps: host
    }
    // ---- analytic normals: n_i = -normalize(d pre_i / d x01_i); rendered N = safe_normalize(sum w_i n_i);
    //      the "normals" output is NormalsShader(N) = (N + 1) / 2
    float nrm[3] = {0.f, 0.f, 0.f};
    float Nv[3] = {0.f, 0.f, 0.f}, Nhat[3] = {0.f, 0.f, 0.f};
    float rN = 0.f;
    if (has_normals) {
        if (act) {
            const float gx = gd[0] * a.dsigma_inv_scale, gy = gd[1] * a.dsigma_inv_scale,
                        gz = gd[2] * a.dsigma_inv_scale;
            const float inv = -1.f / fmaxf(sqrtf(gx * gx + gy * gy + gz * gz), 1e-12f);  // F.normalize eps
            nrm[0] = gx * inv; nrm[1] = gy * inv; nrm[2] = gz * inv;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) Nv[k] = wave_sum(wi * nrm[k]);
        rN = sqrtf(Nv[0] * Nv[0] + Nv[1] * Nv[1] + Nv[2] * Nv[2]);
#pragma unroll
        for (int k = 0; k < 3; ++k) Nhat[k] = Nv[k] / (rN + 1e-10f);  // safe_normalize
        if (a.out_normals && lane == 0) {
#pragma unroll
            for (int k = 0; k < 3; ++k) a.out_normals[3 * (size_t)r + k] = 0.5f * (Nhat[k] + 1.f);
        }
    }
    if (!a.dpre) return;

    // ---- losses
    float dpix[3];
    float l_rgb = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float e = pix[k] - gt[k];
        l_rgb += e * e;
        dpix[k] = a.rgb_mult * 2.f * e * a.inv_rays * (1.f / 3.f);
    }
    l_rgb *= a.inv_rays * (1.f / 3.f);
    // d/dw_i and d/dc_i from the rgb term
    float gw = 0.f;
    float dc[3] = {0.f, 0.f, 0.f};
    if (act) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            gw += dpix[k] * (c[k] - clast[k]);
            dc[k] = dpix[k] * wi;
        }
        if ((uint32_t)lane == S - 1) {
#pragma unroll
            for (int k = 0; k < 3; ++k) dc[k] += dpix[k] * (1.f - acc);
        }
    }
    // distortion (spacing domain): sum_i w_i sum_j w_j |ut_i-ut_j| + sum_i w_i^2 (s_{i+1}-s_i)/3
    float l_dist = 0.f;
    if (a.distortion_mult != 0.f) {
        const float uti = act ? 0.5f * (s0 + s1) : 0.f;
        if (act) ut[lane] = uti;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        float inner = 0.f;
        if (act) {
            for (uint32_t j = 0; j < S; ++j) inner += w[j] * fabsf(uti - ut[j]);
        }
        const float ds = act ? (s1 - s0) : 0.f;
        l_dist = wave_sum(wi * inner + wi * wi * ds * (1.f / 3.f)) * a.inv_rays;
        if (act) gw += a.distortion_mult * a.inv_rays * (2.f * inner + 2.f * wi * ds * (1.f / 3.f));
    }
    // DS-NeRF depth loss on this level
    float l_depth = 0.f;
    if (use_depth) {
        const float z = gt_z * dir_norm;
        const float mask = z > 0.f ? 1.f : 0.f;
        float term = 0.f;
        if (act) {
            const float len = in.t1 - in.t0;
            const float gss = __expf(-((mid - z) * (mid - z)) / (2.f * a.depth_sigma)) * len * mask;
            term = -__logf(wi + kLossEps) * gss;
            gw += a.depth_mult * a.depth_level_div * a.inv_rays * (-gss / (wi + kLossEps));
        }
        l_depth = wave_sum(term) * a.inv_rays * a.depth_level_div;
    }
    // monosdf normal loss on the shaded normals: L1 + (1 - cos) between the L2-normalised vectors
    float l_normal = 0.f;
    if (use_gt_normal) {
        float sh[3], q[3], p[3], dp[3];
        float rs = 0.f, rq = 0.f;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            sh[k] = 0.5f * (Nhat[k] + 1.f);
            q[k] = gtn[k];
            rs += sh[k] * sh[k];
            rq += q[k] * q[k];
        }
        rs = fmaxf(sqrtf(rs), 1e-12f);
        rq = fmaxf(sqrtf(rq), 1e-12f);
        float pdq = 0.f;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            p[k] = sh[k] / rs;
            q[k] /= rq;
            l_normal += fabsf(p[k] - q[k]);
            pdq += p[k] * q[k];
        }
        l_normal = (l_normal + 1.f - pdq) * a.inv_rays;
        // backward: p = sh / |sh|, sh = (Nhat + 1) / 2, Nhat = Nv / (|Nv| + 1e-10)
        float pdp = 0.f;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float e = p[k] - q[k];
            dp[k] = a.normal_mult * a.inv_rays * ((e > 0.f ? 1.f : (e < 0.f ? -1.f : 0.f)) - q[k]);
            pdp += p[k] * dp[k];
        }
        float dN[3], NdN = 0.f;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            dN[k] = 0.5f * (dp[k] - p[k] * pdp) / rs;
            NdN += Nv[k] * dN[k];
        }
        const float den = rN + 1e-10f;
        const float radial = rN > 0.f ? NdN / (rN * den * den) : 0.f;
        if (act) {
#pragma unroll
            for (int k = 0; k < 3; ++k) gw += (dN[k] / den - Nv[k] * radial) * nrm[k];
        }
    }
    if (lane == 0) {
        // 64 shards of 8 floats: thousands of adds to ONE word serialise at the memory side
        // (~88 same-address atomics per us on MI355X); the host sums the shards.
        float* shard = a.losses + 8 * (r & 63u);
        atomicAdd(shard + 0, a.rgb_mult * l_rgb);
        atomicAdd(shard + 1, a.distortion_mult * l_dist);
        atomicAdd(shard + 2, a.depth_mult * l_depth);
        if (l_normal != 0.f) atomicAdd(shard + 6, a.normal_mult * l_normal);
    }
    // ---- dL/dw -> dL/dpre (one chunk: the lane's own gw, wi, Ti; nothing is loaded again)
    float total = 0.f;
    total += act ? gw * wi : 0.f;
    total = wave_sum(total);
    bool overflow = false;
    carry = 0.f;
    const nvo_h16 dpre16 = ray_weights_bwd_chunk(lane, act, keep, gw, wi, Ti, total, carry, a.loss_scale, bf, overflow);
    if (act) ((nvo_h16*)a.dpre)[(so + lane) * a.dpre_stride] = dpre16;
    // lanes whose STORED 16-bit gradient is not zero
    const unsigned long long pre_live = __ballot(act && (dpre16 & 0x7fffu) != 0u);
    if (act) {
        const float fmt_max = bf ? 3.0e38f : 65504.0f;
#pragma unroll
        for (int k = 0; k < 3; ++k) overflow = overflow || !(fabsf(dc[k] * a.loss_scale) <= fmt_max);
    }
    if (a.nonfinite_flag && __ballot(overflow) != 0ull && lane == 0) atomicOr(a.nonfinite_flag, 1u);
    bool rgb_nz = false;
    if (act && a.drgb_stride == 16) {
        // the colour MLP backward reads all 16 columns: one 32-byte row {dr, dg, db, 0 x 13} as two 16-byte stores
        uint4 lo = make_uint4(0u, 0u, 0u, 0u);
        lo.x = nvo_cvt16x2(dc[0] * a.loss_scale, dc[1] * a.loss_scale, bf);
        lo.y = (uint32_t)nvo_cvt16(dc[2] * a.loss_scale, bf);
        uint4* row = reinterpret_cast<uint4*>((nvo_h16*)a.drgb + (so + lane) * 16);
        row[0] = lo;
        row[1] = make_uint4(0u, 0u, 0u, 0u);
        rgb_nz = ((lo.x | lo.y) & 0x7fff7fffu) != 0u;
    } else if (act) {
        nvo_h16* dp = (nvo_h16*)a.drgb + (so + lane) * a.drgb_stride;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            dp[k] = nvo_cvt16(dc[k] * a.loss_scale, bf);
            rgb_nz = rgb_nz || (dp[k] & 0x7fffu) != 0u;
        }
        for (uint32_t k = 3; k < a.drgb_stride; ++k) dp[k] = (nvo_h16)0;
    }
    if (a.tile_live) {  // (the launcher: S % 16 == 0, S <= 64) what the stored 16-bit gradients of each 16-sample tile hold
        const unsigned long long rgb_live = __ballot(rgb_nz);
        uint32_t byte = 0u;
        if (lane < (int)(S >> 4)) {
            const uint32_t sh = 16u * (uint32_t)lane;
            byte = (((rgb_live >> sh) & 0xffffull) != 0ull ? 1u : 0u) | (((pre_live >> sh) & 0xffffull) != 0ull ? 2u : 0u);
            a.tile_live[(so >> 4) + lane] = (uint8_t)byte;
        }
        // slot 7 of the loss shards: the number of tiles that carry any gradient (exact in fp32 up to 2^24) -- what tells the
        // hash grid's backward whether listing the live samples pays (k_live_rows)
        const uint32_t n_live_tiles = (uint32_t)__popcll(__ballot(byte != 0u));
        if (lane == 0 && n_live_tiles) atomicAdd(a.losses + 8 * (r & 63u) + 7, (float)n_live_tiles);
    }
}

// ------------------------------------------------------------------------------------------------
// proposal level: interlevel + depth loss and gradient
// ------------------------------------------------------------------------------------------------
// Workgroups [0, blocks0) serve a0, the rest a1: both proposal levels of a step in ONE launch (nvo_prop_loss_pair) --
// each level alone is a single round of 4096 waves that lasts as long as one ray's dependent chain (17-22 us), so two
// launches cost two chains.
// The paired launch of a 4096-ray step is 8192 waves = the chip's 32 waves per CU: at most 64 VGPRs and 20 KiB of LDS per
// workgroup keep 8 workgroups on a CU and the whole launch resident in ONE round (with 28 waves per CU an eighth of it
// ran as a second round behind a full chain).  w, pre + bias, the interval and its mid-point are only ever read at the
// lane's own samples: registers, one per chunk; g, cy, sb are read at other indices (LDS), and Tr takes the fourth row.
__global__ void __launch_bounds__(kRayBlock) __attribute__((amdgpu_waves_per_eu(8)))
k_prop_loss(nvo_prop_loss_args a0, nvo_prop_loss_args a1, uint32_t blocks0) {
    __shared__ float lds[kRaysPerBlock][4][kMaxS + 4];
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    const bool second = blockIdx.x >= blocks0;  // (uniform)
    nvo_prop_loss_args a = second ? a1 : a0;
    const uint32_t r = (second ? blockIdx.x - blocks0 : blockIdx.x) * kRaysPerBlock + wib;
    if (r >= a.R) return;
    float* Tr = lds[wib][0];
    float* g = lds[wib][1];     // dL/dw of this level (built through a difference array)
    float* cy = lds[wib][2];    // exclusive cumsum of w: cy[0] = 0, cy[j+1] = sum_{<=j} w
    // the two binary searches per main interval walk this level's spacing bins: staged in LDS, each probe
    // is an LDS read instead of a dependent global load
    float* sb = lds[wib][3];
    const uint32_t S = a.S, Sm = a.S_main;
    const size_t so = (size_t)r * S;
    const float* tb = a.tbins + (size_t)r * (S + 1);
    const nvo_h16* pre = (const nvo_h16*)a.pre + so * a.pre_stride;
    const bool bf = a.act_bf16 != 0;
    const float* x01 = a.x01 + 3 * so;
    const bool use_depth = a.depth_mult != 0.f && a.gt_depth;
    // ---- every global load of the ray, before the first wait.  No test of S around them: a chunk past the ray's end asks for
    // the last sample again (one line, the same for all lanes) -- behind a branch the selector's compare is folded into
    // the branch's join and each chunk waits for its own loads before the next chunk's are requested
    RayIn in[kChunks];
    float sbv[kChunks + 1];
    {
        const float* sbg = a.sbins + (size_t)r * (S + 1);
#pragma unroll
        for (int c = 0; c < kChunks; ++c) in[c] = ray_fetch(lane, S, (uint32_t)c * 64u, pre, bf, a.pre_stride, x01, tb);
#pragma unroll
        for (int c = 0; c <= kChunks; ++c) sbv[c] = sbg[min((uint32_t)c * 64u + (uint32_t)lane, S)];
    }
    const uint32_t lm = min((uint32_t)lane, Sm - 1u);  // the lane's main-level interval, or the last one
    const float* cm = a.sbins_main + (size_t)r * (Sm + 1);
    const float cm0 = cm[lm], cm1 = cm[lm + 1];
    const float wm = a.weights_main[(size_t)r * Sm + lm];
    float gt_z = 0.f, dir_norm = 0.f;
    if (use_depth) { gt_z = a.gt_depth[r]; dir_norm = a.directions_norm[r]; }
    if (a.dpre && a.loss_scale_dev) a.loss_scale = *a.loss_scale_dev;
    loads_issued();

#pragma unroll
    for (int c = 0; c <= kChunks; ++c) {
        const uint32_t i = (uint32_t)c * 64u + (uint32_t)lane;
        if (i < S + 1u) sb[i] = sbv[c];
    }
    // ---- weights and their exclusive prefix sum, chunk by chunk with the carries of ray_weights
    float wv[kChunks], xk[kChunks], t0[kChunks], t1[kChunks];
    uint32_t selm = 0u;  // bit c: the selector of the lane's sample of chunk c
    {
        float carry = 0.f, carry_cy = 0.f;
#pragma unroll
        for (int c = 0; c < kChunks; ++c) {
            wv[c] = 0.f; xk[c] = 0.f; t0[c] = in[c].t0; t1[c] = in[c].t1;
            if ((uint32_t)c * 64u < S) {
                const uint32_t i = (uint32_t)c * 64u + (uint32_t)lane;
                float T;
                RayKeep k;
                ray_weights_chunk(lane, in[c], bf, i < S, a.density_bias, carry, wv[c], T, k);
                if (i < S) Tr[i] = T;
                xk[c] = k.x;
                selm |= k.sel ? (1u << c) : 0u;
                const float incl = wave_incl_scan(wv[c], lane) + carry_cy;
                if (i < S) cy[i + 1] = incl;
                carry_cy = nvo_wave_bcast(incl, 63);
            }
        }
    }
    if (lane == 0) cy[0] = 0.f;
    for (uint32_t i = lane; i < S + 2; i += 64) g[i] = 0.f;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

    // ---- interlevel: one main-level interval per lane
    float l_inter = 0.f;
    if ((uint32_t)lane < Sm) {
        int lo = upper_bound(sb, (int)S, cm0) - 1;          // over interval starts sb[0..S)
        lo = min(max(lo, 0), (int)S - 1);
        int hi = upper_bound(sb + 1, (int)S, cm1);          // over interval ends sb[1..S]
        hi = min(max(hi, 0), (int)S - 1);
        const float w_outer = cy[hi + 1] - cy[lo];
        const float diff = wm - w_outer;
        if (diff > 0.f) {
            l_inter = diff * diff / (wm + kLossEps);
            const float coef = a.interlevel_mult * a.inv_rays / (float)Sm;
            const float gi = -2.f * diff / (wm + kLossEps) * coef;  // d/d(w_outer)
            atomicAdd(&g[lo], gi);
            atomicAdd(&g[hi + 1], -gi);
        }
    }
    l_inter = wave_sum(l_inter) * a.inv_rays / (float)Sm;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // difference array -> dL/dw_j (inclusive prefix), plus the depth term
    float l_depth = 0.f;
    const float z = use_depth ? gt_z * dir_norm : 0.f;
    const float mask = z > 0.f ? 1.f : 0.f;
    {
        float carry = 0.f;
#pragma unroll
        for (int c = 0; c < kChunks; ++c) {
            if ((uint32_t)c * 64u < S) {
                const uint32_t i = (uint32_t)c * 64u + (uint32_t)lane;
                const float v = (i < S) ? g[i] : 0.f;
                const float incl = wave_incl_scan(v, lane) + carry;
                carry = nvo_wave_bcast(incl, 63);
                float gi = incl;
                if (i < S && use_depth) {
                    const float midp = 0.5f * (t0[c] + t1[c]);
                    const float len = t1[c] - t0[c];
                    const float gss = __expf(-((midp - z) * (midp - z)) / (2.f * a.depth_sigma)) * len * mask;
                    l_depth += -__logf(wv[c] + kLossEps) * gss;
                    gi += a.depth_mult * a.depth_level_div * a.inv_rays * (-gss / (wv[c] + kLossEps));
                }
                // all lanes finished reading g[i] of this chunk through the scan before it is overwritten
                if (i < S) g[i] = gi;
            }
        }
    }
    l_depth = wave_sum(l_depth) * a.inv_rays * a.depth_level_div;
    if (lane == 0) {
        float* shard = a.losses + 8 * (r & 63u);
        atomicAdd(shard + 0, a.interlevel_mult * l_inter);
        atomicAdd(shard + 1, a.depth_mult * l_depth);
    }
    // value-only call (dpre == NULL): nerfstudio evaluates the interlevel / proposal-level depth terms on EVERY step,
    // also on those where the proposal networks do not train -- the loss values without the gradient pass
    if (a.dpre == nullptr) return;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // ---- dL/dw -> dL/dpre: total of g_i w_i, then per chunk the inclusive prefix -> suffix (exclusive) = total - incl
    float total = 0.f;
#pragma unroll
    for (int c = 0; c < kChunks; ++c) {
        const uint32_t i = (uint32_t)c * 64u + (uint32_t)lane;
        if ((uint32_t)c * 64u < S) total += (i < S) ? g[i] * wv[c] : 0.f;
    }
    total = wave_sum(total);
    bool overflow = false;
    {
        float carry = 0.f;
        nvo_h16* dpre = (nvo_h16*)a.dpre + so * a.dpre_stride;
#pragma unroll
        for (int c = 0; c < kChunks; ++c) {
            if ((uint32_t)c * 64u < S) {
                const uint32_t i = (uint32_t)c * 64u + (uint32_t)lane;
                const bool valid = i < S;
                RayKeep k;
                k.sel = ((selm >> c) & 1u) != 0u;
                k.x = xk[c];
                k.delta = t1[c] - t0[c];
                const float gi = valid ? g[i] : 0.f, Ti = valid ? Tr[i] : 0.f;
                const nvo_h16 d16 = ray_weights_bwd_chunk(lane, valid, k, gi, wv[c], Ti, total, carry, a.loss_scale, bf, overflow);
                if (valid) {
                    if (a.dpre_stride == 16) {
                        // whole 32-byte row {d, 0 x 15} as two 16-byte stores (the MLP backward reads all 16 columns)
                        uint4 lo = make_uint4(0u, 0u, 0u, 0u);
                        lo.x = (uint32_t)d16;
                        uint4* row = reinterpret_cast<uint4*>(dpre + (size_t)i * 16);
                        row[0] = lo;
                        row[1] = make_uint4(0u, 0u, 0u, 0u);
                    } else {
                        dpre[(size_t)i * a.dpre_stride] = d16;
                    }
                }
            }
        }
    }
    if (a.nonfinite_flag && __ballot(overflow) != 0ull && lane == 0) atomicOr(a.nonfinite_flag, 1u);
    if (a.dpre_stride != 16) {
        for (uint32_t i = lane; i < S; i += 64) {
            nvo_h16* dp = (nvo_h16*)a.dpre + (so + i) * a.dpre_stride;
            for (uint32_t k = 1; k < a.dpre_stride; ++k) dp[k] = (nvo_h16)0;
        }
    }
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// exported entry points (group C of include/nerfvo_hip.h)
// ---------------------------------------------------------------------------------------------
extern "C" {

int nvo_weights_pdf(nvo_stream_t stream, const nvo_weights_pdf_args* args) {
    NVO_REQUIRE(args != nullptr, "weights_pdf: args is NULL");
    const nvo_weights_pdf_args a = *args;
    NVO_REQUIRE(a.S >= 1 && a.S <= (uint32_t)kMaxS, "weights_pdf: samples per ray %u not in 1..%d", a.S, kMaxS);
    NVO_REQUIRE(a.S_out <= (uint32_t)kMaxS, "weights_pdf: S_out %u > %d", a.S_out, kMaxS);
    NVO_REQUIRE(a.S_out == 0 || (a.sbins_out && a.tbins_out), "weights_pdf: output bins are NULL");
    NVO_REQUIRE(a.pre && a.x01 && a.tbins && a.weights && a.sbins, "weights_pdf: NULL input");
    NVO_REQUIRE(!a.x01_out || (a.origins && a.directions && a.S_out > 0), "weights_pdf: x01_out needs origins, directions and S_out");
    if (a.R == 0) return NVO_OK;
    NVO_PROF(stream, "weights_pdf[S%u]", a.S);
    NVO_LAUNCH(k_weights_pdf, dim3(nvo_div_up(a.R, kRaysPerBlock)), dim3(kRayBlock), 0, (hipStream_t)stream, a);
    NVO_CHECK_LAUNCH();
    return NVO_OK;
}

int nvo_main_render_loss(nvo_stream_t stream, const nvo_main_loss_args* args) {
    NVO_REQUIRE(args != nullptr, "main_render_loss: args is NULL");
    const nvo_main_loss_args a = *args;
    NVO_REQUIRE(a.S >= 1 && a.S <= 64, "main_render_loss: samples per ray %u not in 1..64", a.S);
    NVO_REQUIRE(a.pre && a.rgb && a.x01 && a.sbins && a.tbins && a.out_rgb && a.out_depth &&
                a.out_accumulation, "main_render_loss: NULL input/output");
    NVO_REQUIRE(!a.dpre || (a.drgb && a.losses && a.gt_rgb && a.drgb_stride >= 3),
                "main_render_loss: training mode needs drgb, losses, gt_rgb");
    NVO_REQUIRE(!a.tile_live || (a.dpre && (a.S & 15u) == 0u), "main_render_loss: tile_live needs training mode and S %% 16 == 0 (S = %u)", a.S);
    if (a.R == 0) return NVO_OK;
    NVO_PROF(stream, "main_render_loss");
    NVO_LAUNCH(k_main_render_loss, dim3(nvo_div_up(a.R, kRaysPerBlock)), dim3(kRayBlock), 0, (hipStream_t)stream, a);
    NVO_CHECK_LAUNCH();
    return NVO_OK;
}

int nvo_prop_loss(nvo_stream_t stream, const nvo_prop_loss_args* args) {
    NVO_REQUIRE(args != nullptr, "prop_loss: args is NULL");
    const nvo_prop_loss_args a = *args;
    NVO_REQUIRE(a.S >= 1 && a.S <= (uint32_t)kMaxS && a.S_main >= 1 && a.S_main <= 64,
                "prop_loss: S=%u (<=%d) S_main=%u (<=64)", a.S, kMaxS, a.S_main);
    NVO_REQUIRE(a.pre && a.x01 && a.sbins && a.tbins && a.sbins_main && a.weights_main && a.losses &&
                (a.dpre == nullptr || a.dpre_stride >= 1), "prop_loss: NULL input/output");
    if (a.R == 0) return NVO_OK;
    NVO_PROF(stream, "prop_loss[S%u]", a.S);
    const uint32_t blocks = nvo_div_up(a.R, kRaysPerBlock);
    NVO_LAUNCH(k_prop_loss, dim3(blocks), dim3(kRayBlock), 0, (hipStream_t)stream, a, a, blocks);
    NVO_CHECK_LAUNCH();
    return NVO_OK;
}

int nvo_prop_loss_pair(nvo_stream_t stream, const nvo_prop_loss_args* args0, const nvo_prop_loss_args* args1) {
    NVO_REQUIRE(args0 != nullptr && args1 != nullptr, "prop_loss_pair: args is NULL");
    for (const nvo_prop_loss_args* p : {args0, args1}) {
        const nvo_prop_loss_args& a = *p;
        NVO_REQUIRE(a.S >= 1 && a.S <= (uint32_t)kMaxS && a.S_main >= 1 && a.S_main <= 64,
                    "prop_loss_pair: S=%u (<=%d) S_main=%u (<=64)", a.S, kMaxS, a.S_main);
        NVO_REQUIRE(a.pre && a.x01 && a.sbins && a.tbins && a.sbins_main && a.weights_main && a.losses &&
                    (a.dpre == nullptr || a.dpre_stride >= 1), "prop_loss_pair: NULL input/output");
    }
    const uint32_t b0 = nvo_div_up(args0->R, kRaysPerBlock), b1 = nvo_div_up(args1->R, kRaysPerBlock);
    if (b0 + b1 == 0) return NVO_OK;
    NVO_PROF(stream, "prop_loss[S%u+S%u]", args0->S, args1->S);
    NVO_LAUNCH(k_prop_loss, dim3(b0 + b1), dim3(kRayBlock), 0, (hipStream_t)stream, *args0, *args1, b0);
    NVO_CHECK_LAUNCH();
    return NVO_OK;
}

}  // extern "C"
