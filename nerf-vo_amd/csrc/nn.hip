// Exact nearest-neighbour query against points binned into a uniform cell grid (DESIGN.md "Nearest-neighbour search"):
// the search behind pointcloud.NeighbourGrid.query, i.e. behind the ICP alignment and the two distance tables of
// evaluation.calculate_metrics_3d.  The reference runs scipy's cKDTree on the CPU.  The rule, for query q (after the
// optional transform x' = ((r0*x + r1*y) + r2*z) + t per row, fp32, the library is built with -ffp-contract=off):
//
//   d2(p)     = (dx*dx + dy*dy) + dz*dz,  d = q - p, in fp32          over ALL M target points p
//   out_dist2 = min d2(p);  out_index = the smallest original index with d2(p) == out_dist2
//   bounded:    only points with d2(p) <= max_dist*max_dist (fp32 product) count; none -> +inf, -1
//
// so the result equals a brute-force evaluation bit for bit and does not depend on the cell size, the grid dimensions or
// the launch shape.  One thread owns one query (no dependency between queries, no atomics); the wrapper sorts the queries
// by their own cell so that the lanes of a wave walk the same cells.
//
// Search: the query's cell c is floor((q - lower) / cell_size) per axis, clamped IN FLOAT to [0, g-1] before the
// conversion to int (a NaN clamps to 0: every input is memory-safe; a query outside the box lands in its nearest cell).
// Ring r = the cells at Chebyshev distance r from c, clipped to the grid; rings are visited in order r = 0, 1, 2, ...
// Cells are stored x fastest, so a row of a ring that lies on its z or y face is ONE run of points
// (cell_start[row + x0] .. cell_start[row + x1 + 1]), and the other rows contribute their two end cells.
//
// Termination after ring r (everything at Chebyshev distance <= r has been seen):
//   * every axis of the grid is covered (c - r <= 0 and c + r >= g - 1): all M points have been seen; or
//   * min(best, max_dist^2) < (kMargin * r * cell_size)^2.
// Argument for the second: take a point p in a cell that has not been seen.  Its cell differs from c by at least r + 1
// on some axis a.  For a query inside the box, in exact arithmetic q lies in cell c and p in its own cell, so
// |q_a - p_a| > r * cell_size.  For a query outside the box, let q' be its projection onto the box: q' lies in cell c
// (that is what the clamp computes), and since the box is convex and p is inside it, |q - p| >= |q' - p| > r * cell_size.
// In fp32 the cell coordinate t = (x - lower) / cell_size carries two roundings (a few ulp where the wrapper's division
// is not correctly rounded): |error| <= 4 * 2^-24 * t <= 2^-12 cells for t <= 1024 cells, for the point and for the
// query alike, so a point or query within that distance of a cell face may be filed one cell off and the true gap is
// at least (r - 2^-11) * cell_size >= r * cell_size * (1 - 2^-11) for r >= 1.  The computed d2 is below the true one by
// at most 5 * 2^-24 relative, and the squared limit carries three more roundings.  kMargin = 1 - 2^-8 leaves a factor
// of about eight over the sum of these; hence every unseen point has a computed d2 > the limit > best, it can neither
// lower the minimum nor tie with it, and in the bounded form it is outside max_dist.  PRECONDITION: at most
// NVO_NN_MAX_CELLS_PER_AXIS = 1024 cells per axis (checked here and by pointcloud.NeighbourGrid, which sizes the grid),
// and every target point inside the grid's box (NeighbourGrid takes the box from the points).
// At r = 0 the limit is 0 and nothing is below it: ring 1 is always visited unless the grid is a single cell.
#include "nvo_kernels.h"
#include "../../include/nerfvo_hip.h"

#include <math.h>

namespace {

constexpr int kBlock = 128;           // 200 000 queries: 1563 workgroups, six per CU
constexpr uint32_t kMaxGrid = 4096;   // grid-stride beyond
constexpr float kMargin = 0.99609375f;  // 1 - 2^-8, see above

struct Best {
    float d2;
    int32_t idx;
};

// points of rows [lo, hi) of the sorted table against q
__device__ __forceinline__ void scan_run(const nvo_nn_args& a, uint32_t lo, uint32_t hi, float qx, float qy, float qz,
                                         float max_d2, Best& b) {
    for (uint32_t j = lo; j < hi; ++j) {
        const float* p = a.points + 3 * (size_t)j;
        const float dx = qx - p[0], dy = qy - p[1], dz = qz - p[2];
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        if (d2 <= b.d2 && d2 <= max_d2) {  // a NaN fails
            const int32_t idx = (int32_t)a.point_index[j];
            if (d2 < b.d2 || b.idx < 0 || idx < b.idx) {
                b.d2 = d2;
                b.idx = idx;
            }
        }
    }
}

__device__ __forceinline__ int cell_of(float x, float lower, float cell_size, uint32_t g) {
    const float t = floorf((x - lower) / cell_size);
    return (int)fminf(fmaxf(t, 0.f), (float)(g - 1u));  // clamp in float: NaN -> 0, +-inf and huge values -> an end cell
}

__global__ void __launch_bounds__(kBlock) k_nn_query(const nvo_nn_args a) {
    const int gx = (int)a.gx, gy = (int)a.gy, gz = (int)a.gz;
    const float max_d2 = a.max_dist * a.max_dist;  // +inf when unbounded
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < a.N; i += (uint64_t)gridDim.x * kBlock) {
        float qx = a.queries[3 * i], qy = a.queries[3 * i + 1], qz = a.queries[3 * i + 2];
        if (a.has_xf) {
            const float x = qx, y = qy, z = qz;
            qx = ((a.xf[0] * x + a.xf[1] * y) + a.xf[2] * z) + a.xf[3];
            qy = ((a.xf[4] * x + a.xf[5] * y) + a.xf[6] * z) + a.xf[7];
            qz = ((a.xf[8] * x + a.xf[9] * y) + a.xf[10] * z) + a.xf[11];
        }
        const int cx = cell_of(qx, a.lower_x, a.cell_size, a.gx);
        const int cy = cell_of(qy, a.lower_y, a.cell_size, a.gy);
        const int cz = cell_of(qz, a.lower_z, a.cell_size, a.gz);
        // the ring that covers the whole grid: at most 1023
        const int r_all = max(max(max(cx, gx - 1 - cx), max(cy, gy - 1 - cy)), max(cz, gz - 1 - cz));
        Best b{INFINITY, -1};
        for (int r = 0;; ++r) {
            const int x0 = max(cx - r, 0), x1 = min(cx + r, gx - 1);
            const int y0 = max(cy - r, 0), y1 = min(cy + r, gy - 1);
            const int z0 = max(cz - r, 0), z1 = min(cz + r, gz - 1);
            for (int z = z0; z <= z1; ++z) {
                const bool z_face = (z == cz - r) || (z == cz + r);
                for (int y = y0; y <= y1; ++y) {
                    const uint32_t row = ((uint32_t)z * a.gy + (uint32_t)y) * a.gx;
                    if (z_face || y == cy - r || y == cy + r) {  // the row lies on the ring: one run of points
                        scan_run(a, a.cell_start[row + x0], a.cell_start[row + x1 + 1], qx, qy, qz, max_d2, b);
                    } else {  // only its two end cells do (r >= 1 here)
                        if (cx - r >= 0) scan_run(a, a.cell_start[row + x0], a.cell_start[row + x0 + 1], qx, qy, qz, max_d2, b);
                        if (cx + r <= gx - 1) scan_run(a, a.cell_start[row + x1], a.cell_start[row + x1 + 1], qx, qy, qz, max_d2, b);
                    }
                }
            }
            if (r >= r_all) break;
            const float lim = kMargin * ((float)r * a.cell_size);
            if (fminf(b.d2, max_d2) < lim * lim) break;
        }
        a.out_dist2[i] = b.d2;
        a.out_index[i] = b.idx;
    }
}

}  // namespace

extern "C" {

int nvo_nn_query(nvo_stream_t stream, const nvo_nn_args* args) {
    NVO_REQUIRE(args != nullptr, "nn_query: args is NULL");
    const nvo_nn_args a = *args;
    NVO_REQUIRE(a.points && a.point_index && a.cell_start && a.queries && a.out_dist2 && a.out_index, "nn_query: NULL argument");
    NVO_REQUIRE(a.N >= 1 && a.N < (1u << 31) && a.M >= 1 && a.M < (1u << 31),
                "nn_query: %u queries and %u points must each be between 1 and 2^31 - 1", a.N, a.M);
    NVO_REQUIRE(a.gx >= 1 && a.gy >= 1 && a.gz >= 1 && a.gx <= NVO_NN_MAX_CELLS_PER_AXIS && a.gy <= NVO_NN_MAX_CELLS_PER_AXIS &&
                    a.gz <= NVO_NN_MAX_CELLS_PER_AXIS && (uint64_t)a.gx * a.gy * a.gz < (1ull << 31),
                "nn_query: grid %u x %u x %u must have 1..%d cells per axis and fewer than 2^31 cells", a.gx, a.gy, a.gz,
                NVO_NN_MAX_CELLS_PER_AXIS);
    NVO_REQUIRE(a.cell_size > 0.f && a.cell_size < INFINITY, "nn_query: cell_size %g must be positive and finite", (double)a.cell_size);
    NVO_REQUIRE(a.max_dist > 0.f, "nn_query: max_dist %g must be positive (INFINITY = unbounded)", (double)a.max_dist);
    const uint32_t blocks = nvo_div_up(a.N, kBlock);
    NVO_PROF(stream, "nn_query");
    NVO_LAUNCH(k_nn_query, dim3(blocks < kMaxGrid ? blocks : kMaxGrid), dim3(kBlock), 0, (hipStream_t)stream, a);
    NVO_CHECK_LAUNCH();
    return NVO_OK;
}

}  // extern "C"
