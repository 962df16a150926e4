// Poisson surface reconstruction on a dense lattice: the second half of the nerfstudio back-end's
// density mesh -- oriented points in, an indicator-like field chi out, whose iso-surface csrc/iso.hip extracts.  The
// reference gets it from Open3D's octree solver on the CPU; this is the project's own dense-lattice rule, stated in
// DESIGN.md section 13 and restated operator by operator in tests/helpers/poisson_oracle.py.
//
// Everything is fp32 with a fixed order of operations (the library is built with -ffp-contract=off) and without float
// atomics, so every kernel equals the oracle bit for bit and two runs give the same bytes.
//
// Lattice: nodes [nx][ny][nz], z fastest, linear index n = (i * ny + j) * nz + k; cells (nx-1)(ny-1)(nz-1), linear index
// (ci * (ny-1) + cj) * (nz-1) + ck.  A field of C channels is planar: [C][nx][ny][nz].  Offsets are 64-bit.
//
// Position of a point on an axis:  g = (p - origin) / h;  c = clamp(floor(g), 0, cells - 1);  t = g - float(c).
// Trilinear weight of corner (dx, dy, dz) of the cell:  w = (ax * ay) * az,  a = d ? t : 1 - t.
//
//   splat      one thread per NODE gathers: the up to eight cells that touch the node in ascending cell index, the points of a
//              cell in their sorted order (cell_start), acc = acc + w * value, from acc = 0.  value = 1 (density W),
//              values[q][c], or values[q][c] / denom[q] (the normal over the density at the point: the vector field V).
//              t is taken against the cell the point was binned into.
//   sample     one thread per POINT: acc = acc + w * field[corner], corners in the order dx, dy, dz (dz fastest), from 0.
//   divergence f = 0.5 * (((Vx[i+1] - Vx[i-1]) + (Vy[j+1] - Vy[j-1])) + (Vz[k+1] - Vz[k-1])) on interior nodes, 0 on the boundary.
//   sweep      red-black Gauss-Seidel half-sweep over the interior nodes with ((i + j + k) & 1) == color:
//              s = ((((chi[i-1] + chi[i+1]) + chi[j-1]) + chi[j+1]) + chi[k-1]) + chi[k+1];  chi = (s - f) * float(1/6).
//   restrict   residual r = f - (s - 6 * chi) and full weighting in one pass: coarse node (I, J, K), interior, takes the 27
//              residuals around fine node (2I, 2J, 2K) -- all interior nodes --
//              line(a, b) = (r[-1] + 2 r[0]) + r[+1] along z, plane(a) = (line[-1] + 2 line[0]) + line[+1] along y,
//              total = (plane[-1] + 2 plane[0]) + plane[+1] along x, coarse f = total * 0.0625 (= 4 / 64); boundary 0.
//   prolong    interior fine node += (sum of the 1, 2, 4 or 8 coarse nodes it lies between, x outermost, z fastest) * weight,
//              weight = 0.5 per odd index; the sum starts from its first term.
//   norm       max |r| over the interior nodes: a maximum has no order, the word is combined with an integer atomic max
//              on the bits of a non-negative float.
//   vcycle     V(2,2): two sweeps (red, then black), restrict, the coarse correction from 0, prolong, two sweeps; the
//              coarsest level gets 32 sweeps.
//
// The stencil kernels stream: lanes run along z, the contiguous axis; a half-sweep reads chi and f and writes half of chi.
// No thread reads a neighbour of a boundary node, whatever the lattice's size against the tile.
#include "nvo_kernels.h"
#include "../../include/nerfvo_hip.h"

#include <math.h>
#include <stdint.h>

namespace {

constexpr int kBlock = 256;
constexpr uint32_t kMaxGrid = 1u << 20;  // flat launches grid-stride beyond
constexpr int kTileZ = 64, kTileY = 4;   // stencil launches: a workgroup is 64 lanes along z by 4 rows
constexpr float kSixth = 0.16666667163372040f;  // float(1 / 6)

struct Dims {
    uint32_t nx, ny, nz;
    __host__ __device__ uint64_t nodes() const { return (uint64_t)nx * ny * nz; }
};

// g, the cell and the fraction of one coordinate
__device__ __forceinline__ float lattice_coord(float p, float origin, float h) { return __fdiv_rn(p - origin, h); }
__device__ __forceinline__ void locate(float g, uint32_t cells, int& c, float& t) {
    const float fl = fminf(fmaxf(floorf(g), 0.f), (float)(cells - 1u));  // clamp in float: NaN -> 0
    c = (int)fl;
    t = g - fl;
}

template <int C>
__global__ void __launch_bounds__(kBlock) k_splat(const nvo_poisson_splat_args a) {
    const uint64_t n_nodes = (uint64_t)a.nx * a.ny * a.nz;
    const int cx = (int)a.nx - 1, cy = (int)a.ny - 1, cz = (int)a.nz - 1;
    for (uint64_t n = (uint64_t)blockIdx.x * kBlock + threadIdx.x; n < n_nodes; n += (uint64_t)gridDim.x * kBlock) {
        const int k = (int)(n % a.nz);
        const uint64_t row = n / a.nz;
        const int j = (int)(row % a.ny), i = (int)(row / a.ny);
        float acc[C];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = 0.f;
        for (int di = 0; di < 2; ++di) {
            const int ii = i - 1 + di;  // di = 0: the node is the cell's upper corner on this axis
            if (ii < 0 || ii >= cx) continue;
            for (int dj = 0; dj < 2; ++dj) {
                const int jj = j - 1 + dj;
                if (jj < 0 || jj >= cy) continue;
                for (int dk = 0; dk < 2; ++dk) {
                    const int kk = k - 1 + dk;
                    if (kk < 0 || kk >= cz) continue;
                    const uint64_t cell = ((uint64_t)ii * (uint64_t)cy + (uint64_t)jj) * (uint64_t)cz + (uint64_t)kk;
                    const uint32_t lo = a.cell_start[cell], hi = a.cell_start[cell + 1];
                    for (uint32_t q = lo; q < hi; ++q) {
                        const float* p = a.points + 3 * (size_t)q;
                        const float tx = lattice_coord(p[0], a.origin[0], a.h) - (float)ii;
                        const float ty = lattice_coord(p[1], a.origin[1], a.h) - (float)jj;
                        const float tz = lattice_coord(p[2], a.origin[2], a.h) - (float)kk;
                        const float ax = di ? 1.f - tx : tx, ay = dj ? 1.f - ty : ty, az = dk ? 1.f - tz : tz;
                        const float w = (ax * ay) * az;
                        if (a.values == nullptr) {
                            acc[0] = acc[0] + w;
                        } else {
#pragma unroll
                            for (int c = 0; c < C; ++c) {
                                float v = a.values[(size_t)C * q + c];
                                if (a.denom != nullptr) v = __fdiv_rn(v, a.denom[q]);
                                acc[c] = acc[c] + w * v;
                            }
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int c = 0; c < C; ++c) a.out[(uint64_t)c * n_nodes + n] = acc[c];
    }
}

template <int C>
__global__ void __launch_bounds__(kBlock) k_sample(const nvo_poisson_sample_args a) {
    const uint64_t n_nodes = (uint64_t)a.nx * a.ny * a.nz;
    for (uint64_t q = (uint64_t)blockIdx.x * kBlock + threadIdx.x; q < a.K; q += (uint64_t)gridDim.x * kBlock) {
        const float* p = a.points + 3 * q;
        int c[3];
        float t[3];
        locate(lattice_coord(p[0], a.origin[0], a.h), a.nx - 1u, c[0], t[0]);
        locate(lattice_coord(p[1], a.origin[1], a.h), a.ny - 1u, c[1], t[1]);
        locate(lattice_coord(p[2], a.origin[2], a.h), a.nz - 1u, c[2], t[2]);
        float acc[C];
#pragma unroll
        for (int ch = 0; ch < C; ++ch) acc[ch] = 0.f;
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
#pragma unroll
            for (int dy = 0; dy < 2; ++dy) {
#pragma unroll
                for (int dz = 0; dz < 2; ++dz) {
                    const float ax = dx ? t[0] : 1.f - t[0], ay = dy ? t[1] : 1.f - t[1], az = dz ? t[2] : 1.f - t[2];
                    const float w = (ax * ay) * az;
                    // c <= cells - 1 on every axis: the corner is a node of the lattice
                    const uint64_t node = ((uint64_t)(c[0] + dx) * a.ny + (uint64_t)(c[1] + dy)) * a.nz + (uint64_t)(c[2] + dz);
#pragma unroll
                    for (int ch = 0; ch < C; ++ch) acc[ch] = acc[ch] + w * a.field[(uint64_t)ch * n_nodes + node];
                }
            }
        }
#pragma unroll
        for (int ch = 0; ch < C; ++ch) a.out[(uint64_t)C * q + ch] = acc[ch];
    }
}

__global__ void __launch_bounds__(kBlock) k_divergence(const float* __restrict__ v, float* __restrict__ f, Dims d) {
    const uint64_t n_nodes = d.nodes();
    const uint64_t sy = d.nz, sx = (uint64_t)d.ny * d.nz;
    for (uint64_t n = (uint64_t)blockIdx.x * kBlock + threadIdx.x; n < n_nodes; n += (uint64_t)gridDim.x * kBlock) {
        const uint32_t k = (uint32_t)(n % d.nz);
        const uint64_t row = n / d.nz;
        const uint32_t j = (uint32_t)(row % d.ny), i = (uint32_t)(row / d.ny);
        float out = 0.f;
        if (i >= 1 && i + 1 < d.nx && j >= 1 && j + 1 < d.ny && k >= 1 && k + 1 < d.nz) {
            const float* vx = v;
            const float* vy = v + n_nodes;
            const float* vz = v + 2 * n_nodes;
            const float dx = vx[n + sx] - vx[n - sx];
            const float dy = vy[n + sy] - vy[n - sy];
            const float dz = vz[n + 1] - vz[n - 1];
            out = 0.5f * ((dx + dy) + dz);
        }
        f[n] = out;
    }
}

// the six neighbours of interior node n in the rule's order
__device__ __forceinline__ float neighbour_sum(const float* chi, uint64_t n, uint64_t sx, uint64_t sy) {
    return ((((chi[n - sx] + chi[n + sx]) + chi[n - sy]) + chi[n + sy]) + chi[n - 1]) + chi[n + 1];
}
__device__ __forceinline__ float residual_at(const float* chi, const float* f, uint64_t n, uint64_t sx, uint64_t sy) {
    return f[n] - (neighbour_sum(chi, n, sx, sy) - 6.f * chi[n]);
}

// grid: (ceil(((nz - 2 + 1) / 2) / 64), ceil((ny - 2) / 4), nx - 2), block (64, 4)
__global__ void __launch_bounds__(kBlock) k_sweep(float* chi, const float* __restrict__ f, Dims d, uint32_t color) {
    const uint32_t i = 1u + blockIdx.z;
    const uint32_t j = 1u + blockIdx.y * kTileY + threadIdx.y;
    if (j + 1 >= d.ny) return;
    const uint32_t k = 1u + 2u * (blockIdx.x * kTileZ + threadIdx.x) + ((i + j + 1u + color) & 1u);
    if (k + 1 >= d.nz) return;
    const uint64_t sy = d.nz, sx = (uint64_t)d.ny * d.nz;
    const uint64_t n = ((uint64_t)i * d.ny + j) * d.nz + k;
    chi[n] = (neighbour_sum(chi, n, sx, sy) - f[n]) * kSixth;
}

// thread per coarse node; grid: (ceil(nzc / 64), ceil(nyc / 4), nxc), block (64, 4).  d: the fine lattice
__global__ void __launch_bounds__(kBlock) k_restrict(const float* __restrict__ chi, const float* __restrict__ f,
                                                     float* __restrict__ coarse, Dims d) {
    const uint32_t nxc = (d.nx - 1u) / 2u + 1u, nyc = (d.ny - 1u) / 2u + 1u, nzc = (d.nz - 1u) / 2u + 1u;
    const uint32_t I = blockIdx.z, J = blockIdx.y * kTileY + threadIdx.y, K = blockIdx.x * kTileZ + threadIdx.x;
    if (I >= nxc || J >= nyc || K >= nzc) return;
    float out = 0.f;
    if (I >= 1 && I + 1 < nxc && J >= 1 && J + 1 < nyc && K >= 1 && K + 1 < nzc) {
        // fine nodes 2I - 1 .. 2I + 1 lie in 1 .. nx - 2: all 27 are interior
        const uint64_t sy = d.nz, sx = (uint64_t)d.ny * d.nz;
        const uint64_t centre = ((uint64_t)(2u * I) * d.ny + 2u * J) * d.nz + 2u * K;
        float plane[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            float line[3];
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                const uint64_t n = centre + (uint64_t)a * sx + (uint64_t)b * sy - sx - sy;  // (2I - 1 + a, 2J - 1 + b, 2K)
                const float r0 = residual_at(chi, f, n - 1, sx, sy);
                const float r1 = residual_at(chi, f, n, sx, sy);
                const float r2 = residual_at(chi, f, n + 1, sx, sy);
                line[b] = (r0 + 2.f * r1) + r2;
            }
            plane[a] = (line[0] + 2.f * line[1]) + line[2];
        }
        out = ((plane[0] + 2.f * plane[1]) + plane[2]) * 0.0625f;
    }
    coarse[((uint64_t)I * nyc + J) * nzc + K] = out;
}

// thread per interior fine node; grid: (ceil((nz - 2) / 64), ceil((ny - 2) / 4), nx - 2), block (64, 4)
__global__ void __launch_bounds__(kBlock) k_prolong(float* __restrict__ chi, const float* __restrict__ coarse, Dims d) {
    const uint32_t i = 1u + blockIdx.z;
    const uint32_t j = 1u + blockIdx.y * kTileY + threadIdx.y;
    const uint32_t k = 1u + blockIdx.x * kTileZ + threadIdx.x;
    if (j + 1 >= d.ny || k + 1 >= d.nz) return;
    const uint32_t nyc = (d.ny - 1u) / 2u + 1u, nzc = (d.nz - 1u) / 2u + 1u;
    const uint32_t ox = i & 1u, oy = j & 1u, oz = k & 1u;  // odd: between coarse nodes i/2 and i/2 + 1 (<= nxc - 1)
    const uint64_t base = ((uint64_t)(i >> 1) * nyc + (j >> 1)) * nzc + (k >> 1);
    float sum = 0.f;  // 0 + first term is the first term
    for (uint32_t a = 0; a <= ox; ++a)
        for (uint32_t b = 0; b <= oy; ++b)
            for (uint32_t c = 0; c <= oz; ++c) sum = sum + coarse[base + ((uint64_t)a * nyc + b) * nzc + c];
    const float w = (ox ? 0.5f : 1.f) * (oy ? 0.5f : 1.f) * (oz ? 0.5f : 1.f);
    const uint64_t n = ((uint64_t)i * d.ny + j) * d.nz + k;
    chi[n] = chi[n] + sum * w;
}

__global__ void __launch_bounds__(kBlock) k_residual_norm(const float* __restrict__ chi, const float* __restrict__ f, Dims d,
                                                          uint32_t* norm_bits) {
    __shared__ float part[kBlock / 64];
    const uint64_t n_nodes = d.nodes();
    const uint64_t sy = d.nz, sx = (uint64_t)d.ny * d.nz;
    float m = 0.f;
    for (uint64_t n = (uint64_t)blockIdx.x * kBlock + threadIdx.x; n < n_nodes; n += (uint64_t)gridDim.x * kBlock) {
        const uint32_t k = (uint32_t)(n % d.nz);
        const uint64_t row = n / d.nz;
        const uint32_t j = (uint32_t)(row % d.ny), i = (uint32_t)(row / d.ny);
        if (i >= 1 && i + 1 < d.nx && j >= 1 && j + 1 < d.ny && k >= 1 && k + 1 < d.nz) {
            const float r = fabsf(residual_at(chi, f, n, sx, sy));
            m = r == r ? fmaxf(m, r) : INFINITY;  // a NaN residual reports as +inf
        }
    }
    for (int s = 32; s >= 1; s >>= 1) m = fmaxf(m, __shfl_xor(m, s, 64));
    if ((threadIdx.x & 63u) == 0u) part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        float b = part[0];
        for (int w = 1; w < kBlock / 64; ++w) b = fmaxf(b, part[w]);
        atomicMax(norm_bits, __float_as_uint(b));  // b >= 0: the order of the bits is the order of the values
    }
}

uint32_t flat_blocks(uint64_t n) {
    const uint64_t b = (n + kBlock - 1) / kBlock;
    return (uint32_t)(b < kMaxGrid ? b : kMaxGrid);
}

bool dims_ok(uint32_t nx, uint32_t ny, uint32_t nz) {
    return nx >= 3 && ny >= 3 && nz >= 3 && nx <= NVO_POISSON_MAX_NODES_PER_AXIS && ny <= NVO_POISSON_MAX_NODES_PER_AXIS &&
           nz <= NVO_POISSON_MAX_NODES_PER_AXIS && (uint64_t)nx * ny * nz < (1ull << 31);
}
#define NVO_POISSON_DIMS(what, nx, ny, nz)                                                                                    \
    NVO_REQUIRE(dims_ok(nx, ny, nz), what ": lattice %u x %u x %u must have 3..%d nodes per axis and fewer than 2^31 nodes", \
                nx, ny, nz, NVO_POISSON_MAX_NODES_PER_AXIS)

const dim3 kTile(kTileZ, kTileY);

void launch_sweep(hipStream_t stream, float* chi, const float* f, Dims d, uint32_t color) {
    const uint32_t pairs = (d.nz - 2u + 1u) / 2u;
    const dim3 grid(nvo_div_up(pairs, kTileZ), nvo_div_up(d.ny - 2u, kTileY), d.nx - 2u);
    NVO_LAUNCH(k_sweep, grid, kTile, 0, stream, chi, f, d, color);
}
void launch_restrict(hipStream_t stream, const float* chi, const float* f, float* coarse, Dims d) {
    const uint32_t nxc = (d.nx - 1u) / 2u + 1u, nyc = (d.ny - 1u) / 2u + 1u, nzc = (d.nz - 1u) / 2u + 1u;
    const dim3 grid(nvo_div_up(nzc, kTileZ), nvo_div_up(nyc, kTileY), nxc);
    NVO_LAUNCH(k_restrict, grid, kTile, 0, stream, chi, f, coarse, d);
}
void launch_prolong(hipStream_t stream, float* chi, const float* coarse, Dims d) {
    const dim3 grid(nvo_div_up(d.nz - 2u, kTileZ), nvo_div_up(d.ny - 2u, kTileY), d.nx - 2u);
    NVO_LAUNCH(k_prolong, grid, kTile, 0, stream, chi, coarse, d);
}
void smooth(hipStream_t stream, float* chi, const float* f, Dims d, int sweeps) {
    for (int s = 0; s < sweeps; ++s) {
        launch_sweep(stream, chi, f, d, 0u);
        launch_sweep(stream, chi, f, d, 1u);
    }
}

bool levels_ok(uint32_t nx, uint32_t ny, uint32_t nz, uint32_t levels) {
    if (levels > 12u) return false;
    const uint32_t c[3] = {nx - 1u, ny - 1u, nz - 1u};
    for (int a = 0; a < 3; ++a)
        if ((c[a] & ((1u << levels) - 1u)) != 0u || (c[a] >> levels) < 2u) return false;
    return true;
}

uint64_t level_floats(uint64_t nodes) { return nvo_round_up(nodes, 4); }  // keeps every level 16-byte aligned

}  // namespace

extern "C" {

int nvo_poisson_splat(nvo_stream_t stream, const nvo_poisson_splat_args* args) {
    NVO_REQUIRE(args != nullptr, "poisson_splat: args is NULL");
    const nvo_poisson_splat_args a = *args;
    NVO_REQUIRE(a.points && a.cell_start && a.out, "poisson_splat: NULL argument");
    NVO_REQUIRE(a.channels == 1 || a.channels == 3, "poisson_splat: %u channels -- 1 or 3", a.channels);
    NVO_REQUIRE(a.values != nullptr || (a.channels == 1 && a.denom == nullptr),
                "poisson_splat: without values the splat is the density: 1 channel, no denom");
    NVO_REQUIRE(a.K >= 1 && a.K < (1u << 31), "poisson_splat: %u points must be between 1 and 2^31 - 1", a.K);
    NVO_POISSON_DIMS("poisson_splat", a.nx, a.ny, a.nz);
    NVO_REQUIRE(a.h > 0.f && a.h < INFINITY, "poisson_splat: h %g must be positive and finite", (double)a.h);
    const dim3 grid(flat_blocks((uint64_t)a.nx * a.ny * a.nz)), block(kBlock);
    NVO_PROF(stream, "poisson_splat");
    if (a.channels == 1) {
        NVO_LAUNCH(k_splat<1>, grid, block, 0, (hipStream_t)stream, a);
    } else {
        NVO_LAUNCH(k_splat<3>, grid, block, 0, (hipStream_t)stream, a);
    }
    NVO_CHECK_LAUNCH();
    return NVO_OK;
}

int nvo_poisson_sample(nvo_stream_t stream, const nvo_poisson_sample_args* args) {
    NVO_REQUIRE(args != nullptr, "poisson_sample: args is NULL");
    const nvo_poisson_sample_args a = *args;
    NVO_REQUIRE(a.field && a.points && a.out, "poisson_sample: NULL argument");
    NVO_REQUIRE(a.channels == 1 || a.channels == 3, "poisson_sample: %u channels -- 1 or 3", a.channels);
    NVO_REQUIRE(a.K >= 1 && a.K < (1u << 31), "poisson_sample: %u points must be between 1 and 2^31 - 1", a.K);
    NVO_POISSON_DIMS("poisson_sample", a.nx, a.ny, a.nz);
    NVO_REQUIRE(a.h > 0.f && a.h < INFINITY, "poisson_sample: h %g must be positive and finite", (double)a.h);
    const dim3 grid(flat_blocks(a.K)), block(kBlock);
    NVO_PROF(stream, "poisson_sample");
    if (a.channels == 1) {
        NVO_LAUNCH(k_sample<1>, grid, block, 0, (hipStream_t)stream, a);
    } else {
        NVO_LAUNCH(k_sample<3>, grid, block, 0, (hipStream_t)stream, a);
    }
    NVO_CHECK_LAUNCH();
    return NVO_OK;
}

int nvo_poisson_divergence(nvo_stream_t stream, const nvo_poisson_level_args* args) {
    NVO_REQUIRE(args != nullptr, "poisson_divergence: args is NULL");
    const nvo_poisson_level_args a = *args;
    NVO_REQUIRE(a.field && a.rhs, "poisson_divergence: field and rhs are needed");
    NVO_POISSON_DIMS("poisson_divergence", a.nx, a.ny, a.nz);
    const Dims d{a.nx, a.ny, a.nz};
    NVO_PROF(stream, "poisson_divergence");
    NVO_LAUNCH(k_divergence, dim3(flat_blocks(d.nodes())), dim3(kBlock), 0, (hipStream_t)stream, a.field, a.rhs, d);
    NVO_CHECK_LAUNCH();
    return NVO_OK;
}

int nvo_poisson_sweep(nvo_stream_t stream, const nvo_poisson_level_args* args) {
    NVO_REQUIRE(args != nullptr, "poisson_sweep: args is NULL");
    const nvo_poisson_level_args a = *args;
    NVO_REQUIRE(a.chi && a.rhs, "poisson_sweep: chi and rhs are needed");
    NVO_REQUIRE(a.color <= 1u, "poisson_sweep: color %u -- 0 (red, (i + j + k) even) or 1 (black)", a.color);
    NVO_POISSON_DIMS("poisson_sweep", a.nx, a.ny, a.nz);
    NVO_PROF(stream, "poisson_sweep");
    launch_sweep((hipStream_t)stream, a.chi, a.rhs, Dims{a.nx, a.ny, a.nz}, a.color);
    NVO_CHECK_LAUNCH();
    return NVO_OK;
}

int nvo_poisson_restrict(nvo_stream_t stream, const nvo_poisson_level_args* args) {
    NVO_REQUIRE(args != nullptr, "poisson_restrict: args is NULL");
    const nvo_poisson_level_args a = *args;
    NVO_REQUIRE(a.chi && a.rhs && a.coarse, "poisson_restrict: chi, rhs and coarse are needed");
    NVO_POISSON_DIMS("poisson_restrict", a.nx, a.ny, a.nz);
    NVO_REQUIRE(levels_ok(a.nx, a.ny, a.nz, 1), "poisson_restrict: lattice %u x %u x %u needs an even number of cells, at least 4, "
                "on every axis", a.nx, a.ny, a.nz);
    NVO_PROF(stream, "poisson_restrict");
    launch_restrict((hipStream_t)stream, a.chi, a.rhs, a.coarse, Dims{a.nx, a.ny, a.nz});
    NVO_CHECK_LAUNCH();
    return NVO_OK;
}

int nvo_poisson_prolong(nvo_stream_t stream, const nvo_poisson_level_args* args) {
    NVO_REQUIRE(args != nullptr, "poisson_prolong: args is NULL");
    const nvo_poisson_level_args a = *args;
    NVO_REQUIRE(a.chi && a.coarse, "poisson_prolong: chi and coarse are needed");
    NVO_POISSON_DIMS("poisson_prolong", a.nx, a.ny, a.nz);
    NVO_REQUIRE(levels_ok(a.nx, a.ny, a.nz, 1), "poisson_prolong: lattice %u x %u x %u needs an even number of cells, at least 4, "
                "on every axis", a.nx, a.ny, a.nz);
    NVO_PROF(stream, "poisson_prolong");
    launch_prolong((hipStream_t)stream, a.chi, a.coarse, Dims{a.nx, a.ny, a.nz});
    NVO_CHECK_LAUNCH();
    return NVO_OK;
}

int nvo_poisson_residual_norm(nvo_stream_t stream, const nvo_poisson_level_args* args) {
    NVO_REQUIRE(args != nullptr, "poisson_residual_norm: args is NULL");
    const nvo_poisson_level_args a = *args;
    NVO_REQUIRE(a.chi && a.rhs && a.norm_bits, "poisson_residual_norm: chi, rhs and norm_bits are needed");
    NVO_POISSON_DIMS("poisson_residual_norm", a.nx, a.ny, a.nz);
    const Dims d{a.nx, a.ny, a.nz};
    const uint64_t blocks = (d.nodes() + kBlock - 1) / kBlock;
    NVO_PROF(stream, "poisson_residual_norm");
    NVO_LAUNCH(k_residual_norm, dim3((uint32_t)(blocks < 4096 ? blocks : 4096)), dim3(kBlock), 0, (hipStream_t)stream, a.chi, a.rhs, d,
               a.norm_bits);
    NVO_CHECK_LAUNCH();
    return NVO_OK;
}

uint64_t nvo_poisson_vcycle_scratch_bytes(uint32_t nx, uint32_t ny, uint32_t nz, uint32_t levels) {
    if (!dims_ok(nx, ny, nz) || !levels_ok(nx, ny, nz, levels)) return 0;
    uint64_t floats = 0;
    for (uint32_t l = 1; l <= levels; ++l)
        floats += 2 * level_floats((uint64_t)(((nx - 1u) >> l) + 1u) * (((ny - 1u) >> l) + 1u) * (((nz - 1u) >> l) + 1u));
    return (floats > 0 ? floats : 4) * sizeof(float);
}

int nvo_poisson_vcycle(nvo_stream_t stream_, const nvo_poisson_vcycle_args* args) {
    NVO_REQUIRE(args != nullptr, "poisson_vcycle: args is NULL");
    const nvo_poisson_vcycle_args a = *args;
    NVO_REQUIRE(a.chi && a.rhs && a.scratch, "poisson_vcycle: NULL argument");
    NVO_REQUIRE(((uintptr_t)a.scratch & 15u) == 0, "poisson_vcycle: scratch must be 16-byte aligned");
    NVO_POISSON_DIMS("poisson_vcycle", a.nx, a.ny, a.nz);
    NVO_REQUIRE(levels_ok(a.nx, a.ny, a.nz, a.levels),
                "poisson_vcycle: %u coarsenings of a lattice of %u x %u x %u nodes -- every axis needs a multiple of 2^levels cells "
                "and at least 2 cells on the coarsest level (levels <= 12)", a.levels, a.nx, a.ny, a.nz);
    hipStream_t stream = (hipStream_t)stream_;
    float* chi[13];
    const float* rhs[13];
    Dims d[13];
    chi[0] = a.chi;
    rhs[0] = a.rhs;
    d[0] = Dims{a.nx, a.ny, a.nz};
    float* s = (float*)a.scratch;
    for (uint32_t l = 1; l <= a.levels; ++l) {
        d[l] = Dims{((a.nx - 1u) >> l) + 1u, ((a.ny - 1u) >> l) + 1u, ((a.nz - 1u) >> l) + 1u};
        chi[l] = s;
        s += level_floats(d[l].nodes());
        rhs[l] = s;
        s += level_floats(d[l].nodes());
    }
    NVO_PROF(stream, "poisson_vcycle");
    for (uint32_t l = 0; l < a.levels; ++l) {
        smooth(stream, chi[l], rhs[l], d[l], NVO_POISSON_SMOOTH_SWEEPS);
        launch_restrict(stream, chi[l], rhs[l], const_cast<float*>(rhs[l + 1]), d[l]);
        // the correction starts from 0 (boundary included: it stays 0)
        const int rc = nvo_zero_async(chi[l + 1], level_floats(d[l + 1].nodes()) * sizeof(float), stream);
        if (rc != NVO_OK) return rc;
    }
    smooth(stream, chi[a.levels], rhs[a.levels], d[a.levels], NVO_POISSON_COARSE_SWEEPS);
    for (uint32_t l = a.levels; l-- > 0;) {
        launch_prolong(stream, chi[l], chi[l + 1], d[l]);
        smooth(stream, chi[l], rhs[l], d[l], NVO_POISSON_SMOOTH_SWEEPS);
    }
    NVO_CHECK_LAUNCH();
    return NVO_OK;
}

}  // extern "C"
