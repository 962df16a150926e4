// Dense bundle adjustment over a window of keyframes (include/nerfvo_hip.h section P).  Kernels:
//
//   k_ba_edge<ACC>      a workgroup owns NVO_BA_TILE pixels of one edge, a lane one pixel.  ba_project is the one copy of
//                       the reprojection; ACC = false stores coordinates and the valid mask and stops there.  ACC = true
//                       forms the residuals, weights and the thirteen Jacobian entries per channel, stores the edge's Ej
//                       row and its contributions to C, wz and Ei per pixel (plain stores into the edge's own rows), and
//                       reduces the 90 block sums: over the wave by DPP (nvo_wave_sum: a fixed tree), over the four waves
//                       in ascending order, into the (edge, tile) slot.
//   k_ba_fold_pixels    per source frame and pixel: C, wz (and Ei of a free source) = the edges' rows added in edge order,
//                       Q = 1 / (C + eta).
//   k_ba_ehat           Ehat[s][a] = (kx[s] is pose a ? Ei[a] : 0) + Ej of the edges kx[s] -> a, edge order.
//   k_ba_fold_blocks    B and v: the (edge, tile) slots added in float64, edges then tiles ascending.
//   k_ba_schur          one wave per (16 x 16 tile, chunk of 1024 pixels, source frame): stages 16 rows x 64 pixels of
//                       Ehat and of Q o Ehat (the extra column n holds Q o wz) in LDS as float64 and issues
//                       v_mfma_f64_16x16x4_f64 over the pixels in ascending order; the tile goes to its own slot.
//   k_ba_schur_fold     S = B + prior - slots in (s, chunk) order; g from column n.
//   k_ba_solve          one workgroup: right-looking Cholesky in place in L (global memory, n <= 192), two substitutions
//                       for dx, one thread per column for L^-1.  A pivot that is not > 0 (NaN included) stops it.
//   k_ba_update_poses / k_ba_update_depths / k_ba_covariance   as the header states them.
//
// Bounds: every frame, pose and edge index a kernel uses comes from the plan's tables, which nvo_ba_plan_create built on
// the host from validated input; every pixel index is compared against HW before a load or a store (loads of lanes past
// the end are clamped to the last pixel and their weight is zero).
#include "nvo_kernels.h"
#include "../../include/nerfvo_hip.h"

#include <math.h>
#include <vector>

namespace {

constexpr int kTile = NVO_BA_TILE, kSums = NVO_BA_SUMS, kChunk = NVO_BA_SCHUR_CHUNK;
constexpr int kOffII = 0, kOffJJ = 21, kOffIJ = 42, kOffVI = 78, kOffVJ = 84;
static_assert(kOffVJ + 6 == kSums, "21 + 21 + 36 + 6 + 6 sums per edge");
constexpr uint32_t kMagic = 0x42414e56u;
constexpr float kZMin = 0.25f, kWScale = 0.001f, kDMin = 0.001f;

struct BaDev {  // by value to every kernel; the pointers address the bound plan's tables
    const int32_t *ii, *jj, *kx, *src_off, *src_edges;
    uint32_t M, K, Kx, t0, P, HW, T;
};

struct BaPlan {
    uint32_t magic;
    uint32_t M, K, t0, t1, P, ht, wd, HW, Kx, T, chunks, npad;
    std::vector<int32_t> table;  // ii[M] jj[M] kx[Kx] src_off[Kx + 1] src_edges[M]
    std::vector<int64_t> kx;
    uint64_t off_part, off_cz, off_cwz, off_eic, off_schur, bytes;
    char* dev;
};

__host__ __device__ inline int sym(int r, int c) { return r * 6 - (r * (r - 1)) / 2 + (c - r); }  // r <= c < 6

struct BaRel {
    float R[9], t[3];
};

__device__ __forceinline__ void quat_R(const float* q, float* R) {
    const float x = q[0], y = q[1], z = q[2], w = q[3];
    R[0] = 1.f - 2.f * (y * y + z * z);
    R[1] = 2.f * (x * y - z * w);
    R[2] = 2.f * (x * z + y * w);
    R[3] = 2.f * (x * y + z * w);
    R[4] = 1.f - 2.f * (x * x + z * z);
    R[5] = 2.f * (y * z - x * w);
    R[6] = 2.f * (x * z - y * w);
    R[7] = 2.f * (y * z + x * w);
    R[8] = 1.f - 2.f * (x * x + y * y);
}

// G_ij = G_j G_i^-1
__device__ __forceinline__ BaRel ba_relative(const float* __restrict__ poses, uint32_t i, uint32_t j) {
    float Ri[9], Rj[9];
    const float* pi = poses + (size_t)i * 7;
    const float* pj = poses + (size_t)j * 7;
    quat_R(pi + 3, Ri);
    quat_R(pj + 3, Rj);
    BaRel g;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) g.R[r * 3 + c] = (Rj[r * 3] * Ri[c * 3] + Rj[r * 3 + 1] * Ri[c * 3 + 1]) + Rj[r * 3 + 2] * Ri[c * 3 + 2];
#pragma unroll
    for (int r = 0; r < 3; ++r) g.t[r] = pj[r] - ((g.R[r * 3] * pi[0] + g.R[r * 3 + 1] * pi[1]) + g.R[r * 3 + 2] * pi[2]);
    return g;
}

struct BaPoint {
    float x, y, z, d, pu, pv;
    bool ok;
};

// the reprojection of pixel (u, v) with inverse depth h through G_ij: the ONE copy, shared by both launchers
__device__ __forceinline__ BaPoint ba_project(const BaRel& g, const float* in, float u, float v, float h) {
    const float fx = in[0], fy = in[1], cx = in[2], cy = in[3];
    const float X0 = (u - cx) / fx, Y0 = (v - cy) / fy;
    BaPoint p;
    p.x = ((g.R[0] * X0 + g.R[1] * Y0) + g.R[2]) + g.t[0] * h;
    p.y = ((g.R[3] * X0 + g.R[4] * Y0) + g.R[5]) + g.t[1] * h;
    p.z = ((g.R[6] * X0 + g.R[7] * Y0) + g.R[8]) + g.t[2] * h;
    p.ok = p.z >= kZMin;
    p.d = p.ok ? 1.f / p.z : 0.f;
    p.pu = fx * (p.d * p.x) + cx;
    p.pv = fy * (p.d * p.y) + cy;
    return p;
}

struct BaIntr {
    float v[4];
};

template <bool ACC>
__global__ void __launch_bounds__(kTile) k_ba_edge(const BaDev pl, const BaIntr in, const float* __restrict__ poses,
                                                   const float* __restrict__ disps, const float* __restrict__ target,
                                                   const float* __restrict__ weight, uint32_t wd, float* __restrict__ coords,
                                                   uint8_t* __restrict__ valid, float* __restrict__ Ej, float* __restrict__ eic,
                                                   float* __restrict__ cz, float* __restrict__ cwz, float* __restrict__ part) {
    __shared__ float red[kTile / NVO_WAVE][kSums];
    const uint32_t e = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
    const uint32_t HW = pl.HW;
    const uint32_t p = tile * kTile + tid;
    const bool live = p < HW;
    const uint32_t pc = live ? p : HW - 1u;
    const uint32_t i = (uint32_t)pl.ii[e], j = (uint32_t)pl.jj[e];
    const BaRel g = ba_relative(poses, i, j);
    const float h = disps[(size_t)i * HW + pc];
    const BaPoint q = ba_project(g, in.v, (float)(pc % wd), (float)(pc / wd), h);
    if (!ACC) {
        if (live) {
            coords[((size_t)e * 2) * HW + p] = q.pu;
            coords[((size_t)e * 2 + 1) * HW + p] = q.pv;
            valid[(size_t)e * HW + p] = q.ok ? 1 : 0;
        }
        return;
    }
    const float fx = in.v[0], fy = in.v[1];
    const float x = q.x, y = q.y, d = q.d, d2 = q.d * q.d;
    float Jj[2][6], Ji[2][6], Jz[2], r[2], w[2];
    Jj[0][0] = fx * (h * d);
    Jj[0][1] = 0.f;
    Jj[0][2] = fx * (-(x * h) * d2);
    Jj[0][3] = fx * (-(x * y) * d2);
    Jj[0][4] = fx * (1.f + (x * x) * d2);
    Jj[0][5] = fx * (-(y * d));
    Jj[1][0] = 0.f;
    Jj[1][1] = fy * (h * d);
    Jj[1][2] = fy * (-(y * h) * d2);
    Jj[1][3] = fy * (-1.f - (y * y) * d2);
    Jj[1][4] = fy * ((x * y) * d2);
    Jj[1][5] = fy * (x * d);
    Jz[0] = fx * (g.t[0] * d - (g.t[2] * x) * d2);
    Jz[1] = fy * (g.t[1] * d - (g.t[2] * y) * d2);
#pragma unroll
    for (int c = 0; c < 2; ++c) {  // J_i = -Ad(G_ij)' J_j
        const float* Jt = Jj[c];
        const float* Jp = Jj[c] + 3;
        float A[3];
        A[0] = Jp[0] - (g.t[1] * Jt[2] - g.t[2] * Jt[1]);
        A[1] = Jp[1] - (g.t[2] * Jt[0] - g.t[0] * Jt[2]);
        A[2] = Jp[2] - (g.t[0] * Jt[1] - g.t[1] * Jt[0]);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            Ji[c][k] = -((g.R[k] * Jt[0] + g.R[3 + k] * Jt[1]) + g.R[6 + k] * Jt[2]);
            Ji[c][3 + k] = -((g.R[k] * A[0] + g.R[3 + k] * A[1]) + g.R[6 + k] * A[2]);
        }
        const float tg = target[((size_t)e * 2 + c) * HW + pc], wt = weight[((size_t)e * 2 + c) * HW + pc];
        r[c] = tg - (c == 0 ? q.pu : q.pv);
        w[c] = (q.ok && live) ? kWScale * wt : 0.f;
    }
    // ---- the edge's own per-pixel rows ----
    {
        const float wJz0 = w[0] * Jz[0], wJz1 = w[1] * Jz[1];
        if (live) {
            cz[(size_t)e * HW + p] = wJz0 * Jz[0] + wJz1 * Jz[1];
            cwz[(size_t)e * HW + p] = wJz0 * r[0] + wJz1 * r[1];
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                eic[((size_t)e * 6 + k) * HW + p] = wJz0 * Ji[0][k] + wJz1 * Ji[1][k];
                Ej[((size_t)e * 6 + k) * HW + p] = wJz0 * Jj[0][k] + wJz1 * Jj[1][k];
            }
        }
    }
    // ---- the 90 block sums: wave tree, then the four waves in order ----
    const uint32_t wave = tid / NVO_WAVE, lane = tid % NVO_WAVE;
    float wJi[2][6], wJj[2][6];
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            wJi[c][k] = w[c] * Ji[c][k];
            wJj[c][k] = w[c] * Jj[c][k];
        }
#pragma unroll
    for (int a = 0; a < 6; ++a) {
#pragma unroll
        for (int b = 0; b < 6; ++b) {
            if (b >= a) {
                const float sii = nvo_wave_sum(wJi[0][a] * Ji[0][b] + wJi[1][a] * Ji[1][b]);
                const float sjj = nvo_wave_sum(wJj[0][a] * Jj[0][b] + wJj[1][a] * Jj[1][b]);
                if (lane == 0) {
                    red[wave][kOffII + sym(a, b)] = sii;
                    red[wave][kOffJJ + sym(a, b)] = sjj;
                }
            }
            const float sij = nvo_wave_sum(wJi[0][a] * Jj[0][b] + wJi[1][a] * Jj[1][b]);
            if (lane == 0) red[wave][kOffIJ + a * 6 + b] = sij;
        }
        const float svi = nvo_wave_sum(wJi[0][a] * r[0] + wJi[1][a] * r[1]);
        const float svj = nvo_wave_sum(wJj[0][a] * r[0] + wJj[1][a] * r[1]);
        if (lane == 0) {
            red[wave][kOffVI + a] = svi;
            red[wave][kOffVJ + a] = svj;
        }
    }
    __syncthreads();
    if (tid < (uint32_t)kSums)
        part[((size_t)e * pl.T + tile) * kSums + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

__global__ void __launch_bounds__(kTile) k_ba_fold_pixels(const BaDev pl, const float* __restrict__ cz, const float* __restrict__ cwz,
                                                          const float* __restrict__ eic, const float* __restrict__ eta,
                                                          float* __restrict__ C, float* __restrict__ wz, float* __restrict__ Q,
                                                          float* __restrict__ Ei) {
    const uint32_t s = blockIdx.y, p = blockIdx.x * kTile + threadIdx.x, HW = pl.HW;
    if (p >= HW) return;
    const int a = pl.kx[s] - (int)pl.t0;
    const bool is_free = a >= 0 && a < (int)pl.P;
    float c = 0.f, z = 0.f, ei[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int n = pl.src_off[s]; n < pl.src_off[s + 1]; ++n) {
        const uint32_t e = (uint32_t)pl.src_edges[n];
        c = c + cz[(size_t)e * HW + p];
        z = z + cwz[(size_t)e * HW + p];
        if (is_free)
#pragma unroll
            for (int k = 0; k < 6; ++k) ei[k] = ei[k] + eic[((size_t)e * 6 + k) * HW + p];
    }
    C[(size_t)s * HW + p] = c;
    wz[(size_t)s * HW + p] = z;
    Q[(size_t)s * HW + p] = 1.f / (c + eta[(size_t)s * HW + p]);
    if (is_free)
#pragma unroll
        for (int k = 0; k < 6; ++k) Ei[((size_t)a * 6 + k) * HW + p] = ei[k];
}

__global__ void __launch_bounds__(kTile) k_ba_ehat(const BaDev pl, const float* __restrict__ Ei, const float* __restrict__ Ej,
                                                   float* __restrict__ Ehat) {
    const uint32_t s = blockIdx.z, a = blockIdx.y, p = blockIdx.x * kTile + threadIdx.x, HW = pl.HW;
    if (p >= HW) return;
    float v[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (pl.kx[s] - (int)pl.t0 == (int)a)
#pragma unroll
        for (int k = 0; k < 6; ++k) v[k] = Ei[((size_t)a * 6 + k) * HW + p];
    for (int n = pl.src_off[s]; n < pl.src_off[s + 1]; ++n) {
        const uint32_t e = (uint32_t)pl.src_edges[n];
        if (pl.jj[e] - (int)pl.t0 == (int)a)
#pragma unroll
            for (int k = 0; k < 6; ++k) v[k] = v[k] + Ej[((size_t)e * 6 + k) * HW + p];
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) Ehat[(((size_t)s * pl.P + a) * 6 + k) * HW + p] = v[k];
}

// block (a, b) of B, or (b == P) the six entries of v[a]
__global__ void __launch_bounds__(64) k_ba_fold_blocks(const BaDev pl, const float* __restrict__ part, double* __restrict__ B,
                                                       double* __restrict__ v) {
    const int a = (int)blockIdx.x, b = (int)blockIdx.y, t = (int)threadIdx.x, P = (int)pl.P;
    const bool is_v = b == P;
    if (t >= (is_v ? 6 : 36)) return;
    const int r = t / 6, c = t % 6;
    const int s_rc = r <= c ? sym(r, c) : sym(c, r);
    double acc = 0.0;
    for (uint32_t e = 0; e < pl.M; ++e) {
        const int i = pl.ii[e] - (int)pl.t0, j = pl.jj[e] - (int)pl.t0;
        if (i != a && j != a) continue;
        for (uint32_t tile = 0; tile < pl.T; ++tile) {
            const float* s = part + ((size_t)e * pl.T + tile) * kSums;
            if (is_v) {
                if (i == a) acc = acc + (double)s[kOffVI + t];
                if (j == a) acc = acc + (double)s[kOffVJ + t];
            } else {
                if (i == a && b == a) acc = acc + (double)s[kOffII + s_rc];
                if (j == a && b == a) acc = acc + (double)s[kOffJJ + s_rc];
                if (i == a && j == b) acc = acc + (double)s[kOffIJ + r * 6 + c];
                if (j == a && i == b) acc = acc + (double)s[kOffIJ + c * 6 + r];
            }
        }
    }
    if (is_v)
        v[(size_t)a * 6 + t] = acc;
    else
        B[((size_t)a * 6 + r) * (6 * (size_t)P) + (size_t)b * 6 + c] = acc;
}

typedef double v4d __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(NVO_WAVE) k_ba_schur(const BaDev pl, const float* __restrict__ Ehat, const float* __restrict__ Q,
                                                       const float* __restrict__ wz, double* __restrict__ slots, uint32_t tiles,
                                                       uint32_t chunks, uint32_t npad) {
    __shared__ double As[16][NVO_WAVE + 1], Bs[16][NVO_WAVE + 1];
    const uint32_t lane = threadIdx.x, s = blockIdx.z, ch = blockIdx.y;
    const uint32_t r0 = (blockIdx.x / tiles) * 16u, c0 = (blockIdx.x % tiles) * 16u;
    const uint32_t HW = pl.HW, n = 6u * pl.P;
    const uint32_t first = ch * kChunk, last = first + kChunk < HW ? first + kChunk : HW;
    const float* E = Ehat + (size_t)s * n * HW;
    v4d acc = {0.0, 0.0, 0.0, 0.0};
    for (uint32_t p0 = first; p0 < last; p0 += NVO_WAVE) {
        const uint32_t p = p0 + lane;
        const bool live = p < last;
        const double q = live ? (double)Q[(size_t)s * HW + p] : 0.0;
#pragma unroll
        for (uint32_t k = 0; k < 16u; ++k) {
            const uint32_t row = r0 + k, col = c0 + k;
            As[k][lane] = (live && row < n) ? (double)E[(size_t)row * HW + p] : 0.0;
            double b = 0.0;
            if (live && col < n)
                b = q * (double)E[(size_t)col * HW + p];
            else if (live && col == n)
                b = q * (double)wz[(size_t)s * HW + p];
            Bs[k][lane] = b;
        }
        __syncthreads();
#pragma unroll
        for (uint32_t kk = 0; kk < NVO_WAVE; kk += 4u) {
            const double a = As[lane & 15u][kk + (lane >> 4)], b = Bs[lane & 15u][kk + (lane >> 4)];
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
        }
        __syncthreads();
    }
    double* out = slots + ((size_t)s * chunks + ch) * npad * npad;
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k)  // D: col = lane & 15, row = (lane >> 4) + 4 k
        out[(size_t)(r0 + (lane >> 4) + 4u * k) * npad + c0 + (lane & 15u)] = acc[k];
}

__global__ void __launch_bounds__(256) k_ba_schur_fold(const double* __restrict__ slots, const double* __restrict__ B,
                                                       const double* __restrict__ v, double prior_weight, double* __restrict__ S,
                                                       double* __restrict__ g, uint32_t n, uint32_t npad, uint32_t n_slots) {
    const uint64_t idx = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (idx >= (uint64_t)n * (n + 1u)) return;
    const uint32_t r = (uint32_t)(idx / (n + 1u)), c = (uint32_t)(idx % (n + 1u));
    double acc = c == n ? v[r] : B[(size_t)r * n + c];
    if (r == c && r < 6u) acc = acc + prior_weight;
    for (uint32_t k = 0; k < n_slots; ++k) acc = acc - slots[((size_t)k * npad + r) * npad + c];
    if (c == n)
        g[r] = acc;
    else
        S[(size_t)r * n + c] = acc;
}

__global__ void __launch_bounds__(256) k_ba_solve(const double* __restrict__ S, const double* __restrict__ g, double* __restrict__ L,
                                                  double* __restrict__ Linv, double* __restrict__ dx, int32_t* __restrict__ status,
                                                  uint32_t n) {
    __shared__ double y[NVO_BA_MAX_NATIVE_N];
    __shared__ double piv;
    __shared__ int bad;
    const uint32_t tid = threadIdx.x;
    if (tid == 0) bad = 0;
    for (uint32_t idx = tid; idx < n * n; idx += 256u) {
        const uint32_t r = idx / n, c = idx % n;
        L[idx] = c <= r ? S[idx] : 0.0;
    }
    __syncthreads();
    for (uint32_t j = 0; j < n; ++j) {
        if (tid == 0) {
            const double d = L[(size_t)j * n + j];
            if (!(d > 0.0)) {
                bad = (int)j + 1;
            } else {
                piv = sqrt(d);
                L[(size_t)j * n + j] = piv;
            }
        }
        __syncthreads();
        if (bad) {
            if (tid == 0) status[0] = bad;
            return;
        }
        const double pv = piv;
        for (uint32_t i = j + 1u + tid; i < n; i += 256u) L[(size_t)i * n + j] = L[(size_t)i * n + j] / pv;
        __syncthreads();
        const uint32_t m = n - j - 1u;
        for (uint32_t idx = tid; idx < m * m; idx += 256u) {
            const uint32_t i = j + 1u + idx / m, k = j + 1u + idx % m;
            if (k <= i) L[(size_t)i * n + k] = L[(size_t)i * n + k] - L[(size_t)i * n + j] * L[(size_t)k * n + j];
        }
        __syncthreads();
    }
    // L y = g, then L' x = y
    for (uint32_t i = tid; i < n; i += 256u) y[i] = g[i];
    __syncthreads();
    for (uint32_t j = 0; j < n; ++j) {
        if (tid == 0) y[j] = y[j] / L[(size_t)j * n + j];
        __syncthreads();
        const double yj = y[j];
        for (uint32_t i = j + 1u + tid; i < n; i += 256u) y[i] = y[i] - L[(size_t)i * n + j] * yj;
        __syncthreads();
    }
    for (uint32_t jj = n; jj-- > 0u;) {
        if (tid == 0) y[jj] = y[jj] / L[(size_t)jj * n + jj];
        __syncthreads();
        const double xj = y[jj];
        for (uint32_t i = tid; i < jj; i += 256u) y[i] = y[i] - L[(size_t)jj * n + i] * xj;
        __syncthreads();
    }
    for (uint32_t i = tid; i < n; i += 256u) dx[i] = y[i];
    // column c of L^-1 by forward substitution of e_c
    for (uint32_t c = tid; c < n; c += 256u) {
        for (uint32_t i = 0; i < c; ++i) Linv[(size_t)i * n + c] = 0.0;
        for (uint32_t i = c; i < n; ++i) {
            double acc = i == c ? 1.0 : 0.0;
            for (uint32_t k = c; k < i; ++k) acc = acc - L[(size_t)i * n + k] * Linv[(size_t)k * n + c];
            Linv[(size_t)i * n + c] = acc / L[(size_t)i * n + i];
        }
    }
    if (tid == 0) status[0] = 0;
}

__global__ void __launch_bounds__(64) k_ba_update_poses(const BaDev pl, float* __restrict__ poses, const double* __restrict__ dx,
                                                        const int32_t* __restrict__ status) {
    const uint32_t a = blockIdx.x * 64u + threadIdx.x;
    if (a >= pl.P || (status && status[0] != 0)) return;
    const double tau[3] = {dx[a * 6], dx[a * 6 + 1], dx[a * 6 + 2]}, phi[3] = {dx[a * 6 + 3], dx[a * 6 + 4], dx[a * 6 + 5]};
    const double th2 = (phi[0] * phi[0] + phi[1] * phi[1]) + phi[2] * phi[2], th = sqrt(th2);
    double ka, kb, kc, qw;
    if (th < 1e-6) {
        ka = 0.5 - th2 / 48.0;
        kb = 0.5 - th2 / 24.0;
        kc = 1.0 / 6.0 - th2 / 120.0;
        qw = 1.0 - th2 / 8.0;
    } else {
        ka = sin(0.5 * th) / th;
        kb = (1.0 - cos(th)) / th2;
        kc = (th - sin(th)) / (th2 * th);
        qw = cos(0.5 * th);
    }
    const double q[4] = {ka * phi[0], ka * phi[1], ka * phi[2], qw};
    // V = I + kb W + kc W W,  W = [phi]x
    const double W[9] = {0.0, -phi[2], phi[1], phi[2], 0.0, -phi[0], -phi[1], phi[0], 0.0};
    double V[9], R[9];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            const double ww = (W[r * 3] * W[c] + W[r * 3 + 1] * W[3 + c]) + W[r * 3 + 2] * W[6 + c];
            V[r * 3 + c] = ((r == c ? 1.0 : 0.0) + kb * W[r * 3 + c]) + kc * ww;
        }
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    R[0] = 1.0 - 2.0 * (y * y + z * z);
    R[1] = 2.0 * (x * y - z * w);
    R[2] = 2.0 * (x * z + y * w);
    R[3] = 2.0 * (x * y + z * w);
    R[4] = 1.0 - 2.0 * (x * x + z * z);
    R[5] = 2.0 * (y * z - x * w);
    R[6] = 2.0 * (x * z - y * w);
    R[7] = 2.0 * (y * z + x * w);
    R[8] = 1.0 - 2.0 * (x * x + y * y);
    float* ps = poses + (size_t)(pl.t0 + a) * 7;
    const double t[3] = {(double)ps[0], (double)ps[1], (double)ps[2]};
    const double b[4] = {(double)ps[3], (double)ps[4], (double)ps[5], (double)ps[6]};
    double tn[3];
    for (int r = 0; r < 3; ++r)
        tn[r] = ((R[r * 3] * t[0] + R[r * 3 + 1] * t[1]) + R[r * 3 + 2] * t[2]) +
                ((V[r * 3] * tau[0] + V[r * 3 + 1] * tau[1]) + V[r * 3 + 2] * tau[2]);
    double qn[4] = {((w * b[0] + x * b[3]) + y * b[2]) - z * b[1], ((w * b[1] - x * b[2]) + y * b[3]) + z * b[0],
                    ((w * b[2] + x * b[1]) - y * b[0]) + z * b[3], ((w * b[3] - x * b[0]) - y * b[1]) - z * b[2]};
    const double nrm = sqrt((qn[0] * qn[0] + qn[1] * qn[1]) + (qn[2] * qn[2] + qn[3] * qn[3]));
    for (int r = 0; r < 3; ++r) ps[r] = (float)tn[r];
    for (int r = 0; r < 4; ++r) ps[3 + r] = (float)(qn[r] / nrm);
}

__global__ void __launch_bounds__(kTile) k_ba_update_depths(const BaDev pl, float* __restrict__ disps, const float* __restrict__ Q,
                                                            const float* __restrict__ wz, const float* __restrict__ Ehat,
                                                            const double* __restrict__ dx, const int32_t* __restrict__ status) {
    const uint32_t s = blockIdx.y, p = blockIdx.x * kTile + threadIdx.x, HW = pl.HW, n = 6u * pl.P;
    if (p >= HW || (status && status[0] != 0)) return;
    const float* E = Ehat + (size_t)s * n * HW;
    float acc = 0.f;
    for (uint32_t r = 0; r < n; ++r) acc = acc + E[(size_t)r * HW + p] * (float)dx[r];
    const float dz = Q[(size_t)s * HW + p] * (wz[(size_t)s * HW + p] - acc);
    float* d = disps + (size_t)pl.kx[s] * HW + p;
    *d = fmaxf(*d + dz, kDMin);
}

__global__ void __launch_bounds__(kTile) k_ba_covariance(const BaDev pl, const float* __restrict__ disps, const float* __restrict__ Q,
                                                         const float* __restrict__ Ehat, const double* __restrict__ Mx,
                                                         float* __restrict__ cov) {
    const uint32_t s = blockIdx.y, p = blockIdx.x * kTile + threadIdx.x, HW = pl.HW, n = 6u * pl.P;
    if (p >= HW) return;
    const float* E = Ehat + (size_t)s * n * HW;
    const double q = (double)Q[(size_t)s * HW + p];
    double sum = 0.0;
    for (uint32_t c0 = 0; c0 < n; c0 += 6u) {  // n is a multiple of 6: six columns of Mx per pass over the rows
        double f[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (uint32_t r = 0; r < n; ++r) {
            const double ev = (double)E[(size_t)r * HW + p];
            const double* m = Mx + (size_t)r * n + c0;
#pragma unroll
            for (int k = 0; k < 6; ++k) f[k] = f[k] + ev * m[k];
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const double qf = q * f[k];
            sum = sum + qf * qf;
        }
    }
    const double d = (double)disps[(size_t)pl.kx[s] * HW + p], d2 = d * d;
    cov[(size_t)pl.kx[s] * HW + p] = (float)((q + sum) / (d2 * d2));
}

const BaPlan* as_plan(const void* h) {
    const BaPlan* pl = (const BaPlan*)h;
    return (pl && pl->magic == kMagic) ? pl : nullptr;
}

BaDev dev_view(const BaPlan& pl) {
    const int32_t* t = (const int32_t*)pl.dev;
    BaDev d;
    d.ii = t;
    d.jj = t + pl.M;
    d.kx = t + 2 * (size_t)pl.M;
    d.src_off = d.kx + pl.Kx;
    d.src_edges = d.src_off + pl.Kx + 1;
    d.M = pl.M, d.K = pl.K, d.Kx = pl.Kx, d.t0 = pl.t0, d.P = pl.P, d.HW = pl.HW, d.T = pl.T;
    return d;
}

#define BA_PLAN(what)                                                                                 \
    const BaPlan* plp = as_plan(plan);                                                                \
    NVO_REQUIRE(plp != nullptr, what ": not a plan of nvo_ba_plan_create");                           \
    NVO_REQUIRE(plp->dev != nullptr, what ": the plan is not bound to device memory (nvo_ba_plan_bind)"); \
    NVO_REQUIRE(args != nullptr, what ": args is NULL");                                              \
    const BaPlan& pl = *plp;                                                                          \
    const nvo_ba_args a = *args;                                                                      \
    const BaDev dv = dev_view(pl)

}  // namespace

extern "C" {

int nvo_ba_plan_create(const int64_t* ii, const int64_t* jj, uint32_t M, uint32_t K, uint32_t t0, uint32_t t1, uint32_t ht,
                       uint32_t wd, void** plan) {
    NVO_REQUIRE(ii && jj && plan, "ba_plan: NULL argument");
    *plan = nullptr;
    NVO_REQUIRE(M >= 1 && M <= 65535u, "ba_plan: %u edges: between 1 and 65535", M);
    NVO_REQUIRE(K >= 2 && K <= 4096u, "ba_plan: %u frames: between 2 and 4096", K);
    NVO_REQUIRE(t0 < t1 && t1 <= K, "ba_plan: free poses [%u, %u) must be a non-empty range inside the %u frames", t0, t1, K);
    NVO_REQUIRE(ht >= 1 && wd >= 1 && (uint64_t)ht * wd <= (1ull << 22), "ba_plan: %u x %u pixels: between 1 and 2^22", wd, ht);
    for (uint32_t e = 0; e < M; ++e) {
        NVO_REQUIRE(ii[e] >= 0 && ii[e] < (int64_t)K, "ba_plan: ii[%u] = %lld is outside the %u frames", e, (long long)ii[e], K);
        NVO_REQUIRE(jj[e] >= 0 && jj[e] < (int64_t)K, "ba_plan: jj[%u] = %lld is outside the %u frames", e, (long long)jj[e], K);
        NVO_REQUIRE(ii[e] != jj[e], "ba_plan: edge %u joins frame %lld to itself", e, (long long)ii[e]);
    }
    BaPlan* pl = new BaPlan();
    pl->magic = kMagic;
    pl->M = M, pl->K = K, pl->t0 = t0, pl->t1 = t1, pl->P = t1 - t0, pl->ht = ht, pl->wd = wd, pl->HW = ht * wd;
    pl->T = nvo_div_up(pl->HW, kTile);
    pl->chunks = nvo_div_up(pl->HW, kChunk);
    pl->npad = 16u * nvo_div_up(6ull * pl->P + 1ull, 16);
    pl->dev = nullptr;
    std::vector<uint32_t> count(K, 0);
    for (uint32_t e = 0; e < M; ++e) count[ii[e]]++;
    for (uint32_t k = 0; k < K; ++k)
        if (count[k]) pl->kx.push_back(k);
    pl->Kx = (uint32_t)pl->kx.size();
    std::vector<int32_t>& t = pl->table;
    t.reserve(3 * (size_t)M + 2 * (size_t)pl->Kx + 1);
    for (uint32_t e = 0; e < M; ++e) t.push_back((int32_t)ii[e]);
    for (uint32_t e = 0; e < M; ++e) t.push_back((int32_t)jj[e]);
    for (int64_t k : pl->kx) t.push_back((int32_t)k);
    int32_t off = 0;
    for (int64_t k : pl->kx) {
        t.push_back(off);
        off += (int32_t)count[k];
    }
    t.push_back(off);
    for (int64_t k : pl->kx)
        for (uint32_t e = 0; e < M; ++e)
            if (ii[e] == k) t.push_back((int32_t)e);
    const uint64_t HW = pl->HW;
    uint64_t at = nvo_round_up(t.size() * sizeof(int32_t), 16);
    pl->off_part = at, at += nvo_round_up((uint64_t)M * pl->T * kSums * sizeof(float), 16);
    pl->off_cz = at, at += nvo_round_up((uint64_t)M * HW * sizeof(float), 16);
    pl->off_cwz = at, at += nvo_round_up((uint64_t)M * HW * sizeof(float), 16);
    pl->off_eic = at, at += nvo_round_up((uint64_t)M * 6 * HW * sizeof(float), 16);
    pl->off_schur = at, at += (uint64_t)pl->Kx * pl->chunks * pl->npad * pl->npad * sizeof(double);
    pl->bytes = at;
    if (pl->bytes >= (1ull << 34) || (uint64_t)pl->npad / 16 * (pl->npad / 16) > 65535ull * 16ull) {
        delete pl;
        nvo_set_error("ba_plan: %u edges, %u free poses and %u x %u pixels need more scratch than one plan takes", M, t1 - t0, wd, ht);
        return NVO_ERR_INVALID;
    }
    *plan = pl;
    return NVO_OK;
}

int nvo_ba_plan_destroy(void* plan) {
    BaPlan* pl = (BaPlan*)as_plan(plan);
    NVO_REQUIRE(pl != nullptr, "ba_plan_destroy: not a plan of nvo_ba_plan_create");
    pl->magic = 0;
    delete pl;
    return NVO_OK;
}

uint64_t nvo_ba_plan_bytes(const void* plan) {
    const BaPlan* pl = as_plan(plan);
    return pl ? pl->bytes : 0;
}

uint32_t nvo_ba_plan_kx(const void* plan, int64_t* kx_out) {
    const BaPlan* pl = as_plan(plan);
    if (!pl) return 0;
    if (kx_out)
        for (uint32_t s = 0; s < pl->Kx; ++s) kx_out[s] = pl->kx[s];
    return pl->Kx;
}

int nvo_ba_plan_bind(nvo_stream_t stream, void* plan, void* device_memory, uint64_t bytes) {
    BaPlan* pl = (BaPlan*)as_plan(plan);
    NVO_REQUIRE(pl != nullptr, "ba_plan_bind: not a plan of nvo_ba_plan_create");
    NVO_REQUIRE(device_memory && ((uintptr_t)device_memory & 15u) == 0u, "ba_plan_bind: device memory must be 16-byte aligned");
    NVO_REQUIRE(bytes >= pl->bytes, "ba_plan_bind: %llu bytes given, nvo_ba_plan_bytes says %llu", (unsigned long long)bytes,
                (unsigned long long)pl->bytes);
    NVO_CHECK_HIP(hipMemcpyAsync(device_memory, pl->table.data(), pl->table.size() * sizeof(int32_t), hipMemcpyHostToDevice,
                                 (hipStream_t)stream));
    pl->dev = (char*)device_memory;
    return NVO_OK;
}

int nvo_ba_reproject(nvo_stream_t stream, const void* plan, const nvo_ba_args* args) {
    BA_PLAN("ba_reproject");
    NVO_REQUIRE(a.poses && a.disps && a.coords && a.valid, "ba_reproject: NULL argument");
    BaIntr in;
    for (int k = 0; k < 4; ++k) in.v[k] = a.intrinsics[k];
    NVO_REQUIRE(in.v[0] != 0.f && in.v[1] != 0.f, "ba_reproject: a focal length is zero");
    NVO_PROF(stream, "ba_reproject");
    NVO_LAUNCH(k_ba_edge<false>, dim3(pl.T, pl.M), dim3(kTile), 0, (hipStream_t)stream, dv, in, a.poses, a.disps, nullptr, nullptr,
               pl.wd, a.coords, a.valid, nullptr, nullptr, nullptr, nullptr, nullptr);
    NVO_CHECK_LAUNCH();
    return NVO_OK;
}

int nvo_ba_accumulate(nvo_stream_t stream, const void* plan, const nvo_ba_args* args) {
    BA_PLAN("ba_accumulate");
    NVO_REQUIRE(a.poses && a.disps && a.target && a.weight && a.eta && a.B && a.v && a.C && a.wz && a.Q && a.Ei && a.Ej,
                "ba_accumulate: NULL argument");
    NVO_REQUIRE((((uintptr_t)a.B | (uintptr_t)a.v) & 7u) == 0u, "ba_accumulate: B and v must be 8-byte aligned");
    BaIntr in;
    for (int k = 0; k < 4; ++k) in.v[k] = a.intrinsics[k];
    NVO_REQUIRE(in.v[0] != 0.f && in.v[1] != 0.f, "ba_accumulate: a focal length is zero");
    hipStream_t st = (hipStream_t)stream;
    float* part = (float*)(pl.dev + pl.off_part);
    float* cz = (float*)(pl.dev + pl.off_cz);
    float* cwz = (float*)(pl.dev + pl.off_cwz);
    float* eic = (float*)(pl.dev + pl.off_eic);
    NVO_PROF(stream, "ba_accumulate");
    // a free pose that is never a source has no Ei row of its own
    NVO_CHECK_HIP(hipMemsetAsync(a.Ei, 0, (size_t)pl.P * 6 * pl.HW * sizeof(float), st));
    NVO_LAUNCH(k_ba_edge<true>, dim3(pl.T, pl.M), dim3(kTile), 0, st, dv, in, a.poses, a.disps, a.target, a.weight, pl.wd, nullptr,
               nullptr, a.Ej, eic, cz, cwz, part);
    NVO_CHECK_LAUNCH();
    NVO_LAUNCH(k_ba_fold_pixels, dim3(pl.T, pl.Kx), dim3(kTile), 0, st, dv, cz, cwz, eic, a.eta, a.C, a.wz, a.Q, a.Ei);
    NVO_CHECK_LAUNCH();
    NVO_LAUNCH(k_ba_fold_blocks, dim3(pl.P, pl.P + 1u), dim3(64), 0, st, dv, part, a.B, a.v);
    NVO_CHECK_LAUNCH();
    if (a.Ehat) {
        NVO_LAUNCH(k_ba_ehat, dim3(pl.T, pl.P, pl.Kx), dim3(kTile), 0, st, dv, a.Ei, a.Ej, a.Ehat);
        NVO_CHECK_LAUNCH();
    }
    return NVO_OK;
}

int nvo_ba_schur(nvo_stream_t stream, const void* plan, const nvo_ba_args* args) {
    BA_PLAN("ba_schur");
    NVO_REQUIRE(a.Ehat && a.Q && a.wz && a.B && a.v && a.S && a.g, "ba_schur: NULL argument");
    NVO_REQUIRE((((uintptr_t)a.B | (uintptr_t)a.v | (uintptr_t)a.S | (uintptr_t)a.g) & 7u) == 0u, "ba_schur: float64 buffers must be 8-byte aligned");
    NVO_REQUIRE(a.prior_weight >= 0.0 && a.prior_weight < INFINITY, "ba_schur: the prior weight must be finite and not negative");
    hipStream_t st = (hipStream_t)stream;
    double* slots = (double*)(pl.dev + pl.off_schur);
    const uint32_t tiles = pl.npad / 16u, n = 6u * pl.P;
    NVO_PROF(stream, "ba_schur");
    NVO_LAUNCH(k_ba_schur, dim3(tiles * tiles, pl.chunks, pl.Kx), dim3(NVO_WAVE), 0, st, dv, a.Ehat, a.Q, a.wz, slots, tiles, pl.chunks,
               pl.npad);
    NVO_CHECK_LAUNCH();
    NVO_LAUNCH(k_ba_schur_fold, dim3(nvo_div_up((uint64_t)n * (n + 1u), 256)), dim3(256), 0, st, slots, a.B, a.v, a.prior_weight, a.S, a.g, n,
               pl.npad, pl.Kx * pl.chunks);
    NVO_CHECK_LAUNCH();
    return NVO_OK;
}

int nvo_ba_solve(nvo_stream_t stream, uint32_t n, const double* S, const double* g, double* L, double* Linv, double* dx,
                 int32_t* status) {
    NVO_REQUIRE(S && g && L && Linv && dx && status, "ba_solve: NULL argument");
    NVO_REQUIRE(n >= 1 && n <= NVO_BA_MAX_NATIVE_N, "ba_solve: a system of %u unknowns; the native solve takes 1 to %d", n,
                NVO_BA_MAX_NATIVE_N);
    NVO_REQUIRE((((uintptr_t)S | (uintptr_t)g | (uintptr_t)L | (uintptr_t)Linv | (uintptr_t)dx) & 7u) == 0u && ((uintptr_t)status & 3u) == 0u,
                "ba_solve: misaligned buffer");
    NVO_PROF(stream, "ba_solve");
    NVO_LAUNCH(k_ba_solve, dim3(1), dim3(256), 0, (hipStream_t)stream, S, g, L, Linv, dx, status, n);
    NVO_CHECK_LAUNCH();
    return NVO_OK;
}

int nvo_ba_update(nvo_stream_t stream, const void* plan, const nvo_ba_args* args) {
    BA_PLAN("ba_update");
    NVO_REQUIRE(a.dx && ((uintptr_t)a.dx & 7u) == 0u, "ba_update: dx is NULL or misaligned");
    NVO_REQUIRE(a.poses || a.disps, "ba_update: neither poses nor disps given");
    NVO_REQUIRE(!a.disps || (a.Q && a.wz && a.Ehat), "ba_update: the depth step needs Q, wz and Ehat");
    hipStream_t st = (hipStream_t)stream;
    NVO_PROF(stream, "ba_update");
    if (a.poses) {
        NVO_LAUNCH(k_ba_update_poses, dim3(nvo_div_up(pl.P, 64)), dim3(64), 0, st, dv, a.poses, a.dx, a.status);
        NVO_CHECK_LAUNCH();
    }
    if (a.disps) {
        NVO_LAUNCH(k_ba_update_depths, dim3(pl.T, pl.Kx), dim3(kTile), 0, st, dv, a.disps, a.Q, a.wz, a.Ehat, a.dx, a.status);
        NVO_CHECK_LAUNCH();
    }
    return NVO_OK;
}

int nvo_ba_covariance(nvo_stream_t stream, const void* plan, const nvo_ba_args* args) {
    BA_PLAN("ba_covariance");
    NVO_REQUIRE(a.disps && a.Q && a.Ehat && a.Mx && a.cov, "ba_covariance: NULL argument");
    NVO_REQUIRE(((uintptr_t)a.Mx & 7u) == 0u, "ba_covariance: Mx must be 8-byte aligned");
    NVO_PROF(stream, "ba_covariance");
    NVO_LAUNCH(k_ba_covariance, dim3(pl.T, pl.Kx), dim3(kTile), 0, (hipStream_t)stream, dv, a.disps, a.Q, a.Ehat, a.Mx, a.cov);
    NVO_CHECK_LAUNCH();
    return NVO_OK;
}

}  // extern "C"
