// Exact k-nearest-neighbour query against points binned into the uniform cell grid of csrc/nn.hip (DESIGN.md "k nearest
// neighbours and the point cloud"): the search behind pointcloud.NeighbourGrid.query_knn and
// pointcloud.remove_statistical_outlier, i.e. behind the outlier removal of the nerfacto point cloud.  The reference gets
// it from Open3D's kd-tree on the CPU.  The rule, for query q (the library is built with -ffp-contract=off):
//
//   d2(p)  = (dx*dx + dy*dy) + dz*dz,  d = q - p, in fp32                 over ALL M target points p
//   result = the k smallest pairs (d2, original index) in lexicographic order: ties on d2 go to the smaller index.
//            out_dist2 [N][k] and out_index [N][k] hold them in that order; with M < k the slots from M on hold +inf, -1.
//   mean   = (((s_0 + s_1) + ...) + s_{c-1}) / float(c),  s_j = sqrt(d2_j), c = min(k, M): fp32, summed in the output's
//            ascending order, square root and division correctly rounded.
//
// so the result equals a brute-force evaluation bit for bit and does not depend on the cell size, the grid dimensions,
// the launch shape or the order of the queries.  One thread owns one query (no dependency between queries, no atomics);
// the wrapper sorts the queries by their own cell so that the lanes of a wave walk the same cells.  With k = 1 the two
// tables are nvo_nn_query's outputs (unbounded, no transform).
//
// Grid, cell rule, clamping of the query's cell, ring order and the cap of NVO_NN_MAX_CELLS_PER_AXIS cells per axis are
// those of csrc/nn.hip; read the comment at its head first.
//
// Termination after ring r (everything at Chebyshev distance <= r cells has been seen):
//   * every axis of the grid is covered (c - r <= 0 and c + r >= g - 1): all M points have been seen; or
//   * the list holds k entries and the d2 of its LAST (k-th) entry is below (kMargin * r * cell_size)^2.
// Argument for the second, which is nn.hip's applied to the k-th entry.  A point p in a cell that has not been seen
// differs from the query's cell by at least r + 1 on some axis, so -- by the argument written out in nn.hip, with the
// same fp32 error budget and the same kMargin = 1 - 2^-8 -- its COMPUTED d2 is above the limit.  The k-th entry's d2 is
// below the limit.  So d2(p) > limit > d2 of the k-th entry >= d2 of every entry: p is strictly farther than all k
// entries of the list, it can neither enter the list nor tie with its last entry, whatever its index.  Stopping as soon
// as the BEST entry is below the limit would be wrong: entries 2..k may still lie beyond the rings seen so far, where
// unseen points can beat them.  A list with fewer than k entries has +inf in its last slot and never stops early.
// At r = 0 the limit is 0 and nothing is below it: ring 1 is always visited unless the grid is a single cell.
//
// The candidate list lives in registers: K slots (K = the smallest of 4, 8, 16, 24, 32 that holds k), kept in DESCENDING
// order so that slot 0 is always the current k-th entry -- the one every candidate is compared with first (early reject:
// a warm list costs one compare per point) and the one the termination test reads.  Slots k .. K-1 hold (-inf, -1),
// below every candidate: the insertion never moves anything past them.  The insertion is a compile-time-unrolled
// compare-and-select over the K slots (no runtime index into the list, hence no scratch); empty slots hold
// (+inf, INT32_MAX), above every candidate, and are written out as (+inf, -1).
#include "nvo_kernels.h"
#include "../../include/nerfvo_hip.h"

#include <math.h>
#include <stdint.h>

namespace {

constexpr int kBlock = 128;
constexpr uint32_t kMaxGrid = 8192;     // grid-stride beyond
constexpr float kMargin = 0.99609375f;  // 1 - 2^-8, as csrc/nn.hip
constexpr int32_t kEmpty = INT32_MAX;   // index of an empty slot: sorts after every point at equal d2

// (d2, idx) < (e2, eidx), lexicographic
__device__ __forceinline__ bool pair_less(float d2, int32_t idx, float e2, int32_t eidx) {
    return d2 < e2 || (d2 == e2 && idx < eidx);
}

template <int K>
struct List {
    float d2[K];     // descending: d2[0] is the k-th entry
    int32_t idx[K];

    __device__ __forceinline__ void init(int k) {
#pragma unroll
        for (int j = 0; j < K; ++j) {
            d2[j] = j < k ? INFINITY : -INFINITY;
            idx[j] = j < k ? kEmpty : -1;
        }
    }

    // (c2, cidx) is known to be below slot 0: it replaces slot 0 (the old k-th entry drops out) and sinks, one
    // compare-and-swap per slot, until its successor is below it.  Each step depends on the one before, which keeps the
    // live temporaries to one pair: the list costs two registers per slot.
    __device__ __forceinline__ void insert(float c2, int32_t cidx) {
        d2[0] = c2;
        idx[0] = cidx;
#pragma unroll
        for (int j = 0; j < K - 1; ++j) {
            const bool swap = pair_less(d2[j], idx[j], d2[j + 1], idx[j + 1]);
            const float a2 = d2[j], b2 = d2[j + 1];
            const int32_t ai = idx[j], bi = idx[j + 1];
            d2[j] = swap ? b2 : a2;
            idx[j] = swap ? bi : ai;
            d2[j + 1] = swap ? a2 : b2;
            idx[j + 1] = swap ? ai : bi;
        }
    }
};

// points of rows [lo, hi) of the sorted table against q
template <int K>
__device__ __forceinline__ void scan_run(const nvo_knn_args& a, uint32_t lo, uint32_t hi, float qx, float qy, float qz, List<K>& l) {
    for (uint32_t j = lo; j < hi; ++j) {
        const float* p = a.points + 3 * (size_t)j;
        const float dx = qx - p[0], dy = qy - p[1], dz = qz - p[2];
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        if (d2 <= l.d2[0]) {  // early reject against the k-th entry; a NaN fails
            const int32_t idx = (int32_t)a.point_index[j];
            if (d2 < l.d2[0] || idx < l.idx[0]) l.insert(d2, idx);
        }
    }
}

__device__ __forceinline__ int cell_of(float x, float lower, float cell_size, uint32_t g) {
    const float t = floorf((x - lower) / cell_size);
    return (int)fminf(fmaxf(t, 0.f), (float)(g - 1u));  // clamp in float: NaN -> 0, +-inf and huge values -> an end cell
}

template <int K>
__global__ void __launch_bounds__(kBlock) k_knn_query(const nvo_knn_args a) {
    const int gx = (int)a.gx, gy = (int)a.gy, gz = (int)a.gz;
    const int k = (int)a.k;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < a.N; i += (uint64_t)gridDim.x * kBlock) {
        const float qx = a.queries[3 * i], qy = a.queries[3 * i + 1], qz = a.queries[3 * i + 2];
        const int cx = cell_of(qx, a.lower_x, a.cell_size, a.gx);
        const int cy = cell_of(qy, a.lower_y, a.cell_size, a.gy);
        const int cz = cell_of(qz, a.lower_z, a.cell_size, a.gz);
        // the ring that covers the whole grid: at most 1023
        const int r_all = max(max(max(cx, gx - 1 - cx), max(cy, gy - 1 - cy)), max(cz, gz - 1 - cz));
        List<K> l;
        l.init(k);
        for (int r = 0;; ++r) {
            const int x0 = max(cx - r, 0), x1 = min(cx + r, gx - 1);
            const int y0 = max(cy - r, 0), y1 = min(cy + r, gy - 1);
            const int z0 = max(cz - r, 0), z1 = min(cz + r, gz - 1);
            for (int z = z0; z <= z1; ++z) {
                const bool z_face = (z == cz - r) || (z == cz + r);
                for (int y = y0; y <= y1; ++y) {
                    const uint32_t row = ((uint32_t)z * a.gy + (uint32_t)y) * a.gx;
                    // up to two runs of points per row, scanned by ONE copy of the loop (the unrolled insertion is large)
                    uint32_t lo0 = 0, hi0 = 0, lo1 = 0, hi1 = 0;
                    if (z_face || y == cy - r || y == cy + r) {  // the row lies on the ring: one run of points
                        lo0 = a.cell_start[row + x0];
                        hi0 = a.cell_start[row + x1 + 1];
                    } else {  // only its two end cells do (r >= 1 here)
                        if (cx - r >= 0) {
                            lo0 = a.cell_start[row + x0];
                            hi0 = a.cell_start[row + x0 + 1];
                        }
                        if (cx + r <= gx - 1) {
                            lo1 = a.cell_start[row + x1];
                            hi1 = a.cell_start[row + x1 + 1];
                        }
                    }
#pragma unroll 1
                    for (int s = 0; s < 2; ++s) scan_run<K>(a, s ? lo1 : lo0, s ? hi1 : hi0, qx, qy, qz, l);
                }
            }
            if (r >= r_all) break;
            const float lim = kMargin * ((float)r * a.cell_size);
            if (l.d2[0] < lim * lim) break;  // the k-th entry; +inf while the list is not full
        }
        // slot j is entry k - 1 - j of the ascending output
        if (a.out_dist2) {
            // one base address per table and a constant offset per slot
            float* od = a.out_dist2 + ((size_t)i * (size_t)k + (size_t)(k - 1));
            int32_t* oi = a.out_index + ((size_t)i * (size_t)k + (size_t)(k - 1));
#pragma unroll
            for (int j = 0; j < K; ++j) {
                if (j < k) {
                    od[-j] = l.d2[j];
                    oi[-j] = l.idx[j] == kEmpty ? -1 : l.idx[j];
                }
            }
        }
        if (a.out_mean_dist) {
            float sum = 0.f;  // 0 + s_0 is s_0
            int c = 0;
#pragma unroll
            for (int j = K - 1; j >= 0; --j) {
                if (j < k && l.idx[j] != kEmpty) {
                    sum = sum + __fsqrt_rn(l.d2[j]);
                    ++c;
                }
            }
            a.out_mean_dist[i] = __fdiv_rn(sum, (float)c);  // M >= 1: c >= 1
        }
    }
}

}  // namespace

extern "C" {

int nvo_knn_query(nvo_stream_t stream, const nvo_knn_args* args) {
    NVO_REQUIRE(args != nullptr, "knn_query: args is NULL");
    const nvo_knn_args a = *args;
    NVO_REQUIRE(a.points && a.point_index && a.cell_start && a.queries, "knn_query: NULL argument");
    NVO_REQUIRE((a.out_dist2 != nullptr) == (a.out_index != nullptr),
                "knn_query: out_dist2 and out_index are one table: pass both or neither");
    NVO_REQUIRE(a.out_dist2 || a.out_mean_dist, "knn_query: both outputs are NULL: pass the table pair, out_mean_dist or both");
    NVO_REQUIRE(a.k >= 1 && a.k <= NVO_KNN_MAX_K, "knn_query: k = %u must be between 1 and NVO_KNN_MAX_K = %d", a.k, NVO_KNN_MAX_K);
    NVO_REQUIRE(a.N >= 1 && a.N < (1u << 31) && a.M >= 1 && a.M < (1u << 31),
                "knn_query: %u queries and %u points must each be between 1 and 2^31 - 1", a.N, a.M);
    NVO_REQUIRE(a.gx >= 1 && a.gy >= 1 && a.gz >= 1 && a.gx <= NVO_NN_MAX_CELLS_PER_AXIS && a.gy <= NVO_NN_MAX_CELLS_PER_AXIS &&
                    a.gz <= NVO_NN_MAX_CELLS_PER_AXIS && (uint64_t)a.gx * a.gy * a.gz < (1ull << 31),
                "knn_query: grid %u x %u x %u must have 1..%d cells per axis and fewer than 2^31 cells", a.gx, a.gy, a.gz,
                NVO_NN_MAX_CELLS_PER_AXIS);
    NVO_REQUIRE(a.cell_size > 0.f && a.cell_size < INFINITY, "knn_query: cell_size %g must be positive and finite", (double)a.cell_size);
    const uint32_t blocks = nvo_div_up(a.N, kBlock);
    const dim3 grid(blocks < kMaxGrid ? blocks : kMaxGrid), block(kBlock);
    NVO_PROF(stream, "knn_query");
    if (a.k <= 4) {
        NVO_LAUNCH(k_knn_query<4>, grid, block, 0, (hipStream_t)stream, a);
    } else if (a.k <= 8) {
        NVO_LAUNCH(k_knn_query<8>, grid, block, 0, (hipStream_t)stream, a);
    } else if (a.k <= 16) {
        NVO_LAUNCH(k_knn_query<16>, grid, block, 0, (hipStream_t)stream, a);
    } else if (a.k <= 24) {
        NVO_LAUNCH(k_knn_query<24>, grid, block, 0, (hipStream_t)stream, a);
    } else {
        NVO_LAUNCH(k_knn_query<32>, grid, block, 0, (hipStream_t)stream, a);
    }
    NVO_CHECK_LAUNCH();
    return NVO_OK;
}

}  // extern "C"
