// Iso-surface of a scalar field on a regular lattice: marching tetrahedra in which every vertex is
// OWNED by its lattice edge, so that no merge step, no atomics and no ordering between workgroups are needed.
//
// Rule (include/nerfvo_hip.h section J; tests/helpers/iso_oracle.py restates it in numpy):
//   inside(p) = values[p] > threshold                                   (a NaN is outside)
//   cube (named by its minimum corner) is active when it exists and its eight corners are valid
//   edge (a, kind): b = a + kIsoKind[kind]; it carries a vertex when b is in the lattice, inside(a) != inside(b) and an
//                   active cube has both a and b among its corners
//   vertex order: ascending (linear index of a, kind)
//   position:     t = clamp((threshold - va) / (vb - va), 0, 1); g = float(a_axis) + (d_axis ? t : 0);
//                 out = lower_axis + g * step_axis                      (fp32 as written, -ffp-contract=off)
//   faces:        active cubes ascending, tetrahedra 0..5, the triangles of kIsoTriEdge at (tet, case), winding applied
//
// Structure: a workgroup owns `points_per_workgroup` CONSECUTIVE lattice points and walks them 256 at a time, so ranks
// inside a workgroup follow the rule's order.
//   k_iso_count: per point the 7-bit mask of the cut edges it owns, the rank of its first vertex inside the workgroup,
//                the triangle count of its cube; per workgroup the totals.
//   (caller: exclusive prefix sums of the totals)
//   k_iso_emit:  vertices from (base of the workgroup + rank); a triangle finds the id of a vertex from its owner q:
//                base[q / points_per_workgroup] + rank[q] + popc(mask[q] below kind).
// The 8 samples a point reads are its cube's 8 corners and at the same time the far ends of its 7 edge kinds.
#include "nvo_kernels.h"
#include "../../include/nerfvo_hip.h"
#include "iso_dev.h"

namespace {

constexpr uint32_t kBlock = 256;
constexpr uint32_t kMinPoints = 64, kMaxPoints = 1u << 22;  // per workgroup: at most 2^14 rounds of 256

struct IsoScratch {
    int64_t* totals;   // [2][G]
    uint32_t* vrank;   // [n]
    uint8_t* mask;     // [n]
    uint8_t* tcount;   // [n]
};

// byte offsets of the four parts (each a multiple of 16) and the total
__host__ __device__ inline void iso_layout(uint64_t n, uint64_t groups, uint64_t off[5]) {
    off[0] = 0;
    off[1] = off[0] + ((2 * groups * sizeof(int64_t) + 15) / 16) * 16;
    off[2] = off[1] + ((n * sizeof(uint32_t) + 15) / 16) * 16;
    off[3] = off[2] + ((n + 15) / 16) * 16;
    off[4] = off[3] + ((n + 15) / 16) * 16;
}

__device__ __forceinline__ IsoScratch iso_scratch(void* base, uint64_t n, uint64_t groups) {
    uint64_t off[5];
    iso_layout(n, groups, off);
    uint8_t* p = (uint8_t*)base;
    IsoScratch s;
    s.totals = (int64_t*)(p + off[0]);
    s.vrank = (uint32_t*)(p + off[1]);
    s.mask = p + off[2];
    s.tcount = p + off[3];
    return s;
}

// bit m: corner m of the cube at (i, j, k) is inside; bit 8 + m: it is in the lattice.  Corner 0 is the point itself.
__device__ __forceinline__ uint32_t corner_bits(const nvo_iso_args& a, uint32_t p, uint32_t i, uint32_t j, uint32_t k) {
    uint32_t bits = 0;
#pragma unroll
    for (uint32_t m = 0; m < 8; ++m) {
        const uint32_t dx = kIsoCorner[m][0], dy = kIsoCorner[m][1], dz = kIsoCorner[m][2];
        if (i + dx < a.nx && j + dy < a.ny && k + dz < a.nz) {
            const size_t q = (size_t)p + ((size_t)dx * a.ny + dy) * a.nz + dz;
            bits |= (a.values[q] > a.threshold ? 1u : 0u) << m;
            bits |= 1u << (8 + m);
        }
    }
    return bits;
}

// bit (dx+1)*9 + (dy+1)*3 + (dz+1): the neighbour at that offset is in the lattice and valid
__device__ __forceinline__ uint32_t neighbourhood(const nvo_iso_args& a, uint32_t i, uint32_t j, uint32_t k) {
    uint32_t nb = 0;
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx)
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dz = -1; dz <= 1; ++dz) {
                const int64_t x = (int64_t)i + dx, y = (int64_t)j + dy, z = (int64_t)k + dz;
                bool ok = x >= 0 && y >= 0 && z >= 0 && x < (int64_t)a.nx && y < (int64_t)a.ny && z < (int64_t)a.nz;
                if (ok && a.valid != nullptr) ok = a.valid[((size_t)x * a.ny + (size_t)y) * a.nz + (size_t)z] != 0;
                nb |= (ok ? 1u : 0u) << ((dx + 1) * 9 + (dy + 1) * 3 + (dz + 1));
            }
    return nb;
}

__global__ void __launch_bounds__(kBlock) k_iso_count(const nvo_iso_args a, uint32_t n, uint32_t groups) {
    __shared__ uint32_t lds[4];
    const IsoScratch s = iso_scratch(a.scratch, n, groups);
    const uint64_t first = (uint64_t)blockIdx.x * a.points_per_workgroup;
    const uint32_t p0 = (uint32_t)first;  // first < n < 2^31
    const uint32_t p1 = (uint32_t)(first + a.points_per_workgroup < n ? first + a.points_per_workgroup : n);
    uint32_t vrun = 0, trun = 0;
    for (uint32_t base = p0; base < p1; base += kBlock) {  // at most points_per_workgroup / 256 rounds
        const uint32_t p = base + threadIdx.x;
        uint32_t mask = 0, tris = 0;
        if (p < p1) {
            const uint32_t k = p % a.nz, ij = p / a.nz, j = ij % a.ny, i = ij / a.ny;
            const uint32_t bits = corner_bits(a, p, i, j, k);
            const uint32_t in = bits & 0xFFu, have = bits >> 8;
            const uint32_t differ = ((bits & 1u) ? ~in : in) & have & 0xFEu;  // corners on the other side than the point
            if (differ != 0u) iso_classify(in, differ, neighbourhood(a, i, j, k), mask, tris);
        }
        uint32_t vtot, ttot;
        const uint32_t vex = block_excl_scan(__popc(mask), lds, vtot);
        (void)block_excl_scan(tris, lds, ttot);
        if (p < p1) {
            s.vrank[p] = vrun + vex;
            s.mask[p] = (uint8_t)mask;
            s.tcount[p] = (uint8_t)tris;
        }
        vrun += vtot;
        trun += ttot;
    }
    if (threadIdx.x == 0) {
        s.totals[blockIdx.x] = (int64_t)vrun;
        s.totals[(size_t)groups + blockIdx.x] = (int64_t)trun;
    }
}

__global__ void __launch_bounds__(kBlock) k_iso_emit(const nvo_iso_args a, uint32_t n, uint32_t groups) {
    __shared__ uint32_t lds[4];
    const IsoScratch s = iso_scratch(a.scratch, n, groups);
    const uint64_t first = (uint64_t)blockIdx.x * a.points_per_workgroup;
    const uint32_t p0 = (uint32_t)first;
    const uint32_t p1 = (uint32_t)(first + a.points_per_workgroup < n ? first + a.points_per_workgroup : n);
    const uint64_t vbase = (uint64_t)a.vertex_base[blockIdx.x], fbase = (uint64_t)a.face_base[blockIdx.x];
    uint32_t trun = 0;
    for (uint32_t base = p0; base < p1; base += kBlock) {
        const uint32_t p = base + threadIdx.x;
        uint32_t mask = 0, tris = 0, i = 0, j = 0, k = 0;
        if (p < p1) {
            mask = s.mask[p];
            tris = s.tcount[p];
            k = p % a.nz;
            const uint32_t ij = p / a.nz;
            j = ij % a.ny;
            i = ij / a.ny;
        }
        if (mask != 0u) {
            uint64_t id = vbase + s.vrank[p];
            const float va = a.values[p];
            for (uint32_t kind = 0; kind < 7; ++kind) {
                if (!((mask >> kind) & 1u)) continue;
                const uint32_t dx = kIsoKind[kind][0], dy = kIsoKind[kind][1], dz = kIsoKind[kind][2];
                const float vb = a.values[(size_t)p + ((size_t)dx * a.ny + dy) * a.nz + dz];
                const float3 pos = iso_vertex(i, j, k, dx, dy, dz, iso_cut(va, vb, a.threshold), a.lower, a.step);
                if (id < a.n_vertices) {  // (always, when vertex_base is the prefix sum of this scratch's totals)
                    float* o = a.vertices + (size_t)id * 3;
                    o[0] = pos.x;
                    o[1] = pos.y;
                    o[2] = pos.z;
                }
                ++id;
            }
        }
        uint32_t ttot;
        const uint32_t tex = block_excl_scan(tris, lds, ttot);
        if (tris != 0u) {  // the cube at p is active: all eight corners are in the lattice
            uint32_t in = 0;
#pragma unroll
            for (uint32_t m = 0; m < 8; ++m) {
                const size_t q = (size_t)p + ((size_t)kIsoCorner[m][0] * a.ny + kIsoCorner[m][1]) * a.nz + kIsoCorner[m][2];
                in |= (a.values[q] > a.threshold ? 1u : 0u) << m;
            }
            iso_emit_faces(in, fbase + trun + tex, a.n_faces, a.faces, [&] __device__(uint32_t oc, uint32_t kind) {
                const uint32_t q = p + (kIsoCorner[oc][0] * a.ny + kIsoCorner[oc][1]) * a.nz + kIsoCorner[oc][2];  // < n
                const uint32_t below = (uint32_t)s.mask[q] & ((1u << kind) - 1u);
                return (int32_t)((uint64_t)a.vertex_base[q / a.points_per_workgroup] + s.vrank[q] + __popc(below));
            });
        }
        trun += ttot;
    }
}

__global__ void __launch_bounds__(kBlock) k_lattice_positions(const nvo_lattice_args a) {
    const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
    if (r >= a.count) return;
    const uint64_t p = a.first + r;
    const uint32_t k = (uint32_t)(p % a.nz);
    const uint64_t ij = p / a.nz;
    const uint32_t j = (uint32_t)(ij % a.ny), i = (uint32_t)(ij / a.ny);
    float* o = a.positions + (size_t)r * 3;
    o[0] = a.lower[0] + (float)i * a.step[0];
    o[1] = a.lower[1] + (float)j * a.step[1];
    o[2] = a.lower[2] + (float)k * a.step[2];
}

int iso_check(const nvo_iso_args& a, const char* what, uint64_t* n, uint64_t* groups) {
    NVO_REQUIRE(a.values && a.scratch, "%s: NULL values or scratch", what);
    NVO_REQUIRE(a.nx >= 2 && a.ny >= 2 && a.nz >= 2 && a.nx < (1u << 31) && a.ny < (1u << 31) && a.nz < (1u << 31) &&
                    (uint64_t)a.nx * a.ny < (1ull << 31) && (uint64_t)a.nx * a.ny * a.nz < (1ull << 31),
                "%s: lattice %u x %u x %u must have at least 2 samples per axis and fewer than 2^31 in all", what, a.nx, a.ny, a.nz);
    NVO_REQUIRE(a.points_per_workgroup >= kMinPoints && a.points_per_workgroup <= kMaxPoints,
                "%s: points_per_workgroup %u not in %u..%u", what, a.points_per_workgroup, kMinPoints, kMaxPoints);
    NVO_REQUIRE(((uintptr_t)a.scratch & 15u) == 0u, "%s: scratch must be 16-byte aligned", what);
    *n = (uint64_t)a.nx * a.ny * a.nz;
    *groups = (*n + a.points_per_workgroup - 1) / a.points_per_workgroup;
    return NVO_OK;
}

}  // namespace

extern "C" {

uint64_t nvo_iso_workgroups(uint32_t nx, uint32_t ny, uint32_t nz, uint32_t points_per_workgroup) {
    if (points_per_workgroup == 0) return 0;
    const uint64_t n = (uint64_t)nx * ny * nz;
    return (n + points_per_workgroup - 1) / points_per_workgroup;
}

uint64_t nvo_iso_scratch_bytes(uint32_t nx, uint32_t ny, uint32_t nz, uint32_t points_per_workgroup) {
    const uint64_t n = (uint64_t)nx * ny * nz, groups = nvo_iso_workgroups(nx, ny, nz, points_per_workgroup);
    uint64_t off[5];
    iso_layout(n, groups, off);
    return off[4];
}

int nvo_iso_count(nvo_stream_t stream, const nvo_iso_args* args) {
    NVO_REQUIRE(args != nullptr, "iso_count: args is NULL");
    const nvo_iso_args a = *args;
    uint64_t n, groups;
    if (int rc = iso_check(a, "iso_count", &n, &groups)) return rc;
    NVO_PROF(stream, "iso_count");
    NVO_LAUNCH(k_iso_count, dim3((uint32_t)groups), dim3(kBlock), 0, (hipStream_t)stream, a, (uint32_t)n, (uint32_t)groups);
    NVO_CHECK_LAUNCH();
    return NVO_OK;
}

int nvo_iso_emit(nvo_stream_t stream, const nvo_iso_args* args) {
    NVO_REQUIRE(args != nullptr, "iso_emit: args is NULL");
    const nvo_iso_args a = *args;
    uint64_t n, groups;
    if (int rc = iso_check(a, "iso_emit", &n, &groups)) return rc;
    if (int rc = iso_counts_check("iso_emit", a.n_vertices, a.n_faces)) return rc;
    if (a.n_vertices == 0 && a.n_faces == 0) return NVO_OK;
    NVO_REQUIRE(a.vertex_base && a.face_base && (a.vertices || a.n_vertices == 0) && (a.faces || a.n_faces == 0),
                "iso_emit: NULL vertex_base, face_base, vertices or faces");
    NVO_PROF(stream, "iso_emit");
    NVO_LAUNCH(k_iso_emit, dim3((uint32_t)groups), dim3(kBlock), 0, (hipStream_t)stream, a, (uint32_t)n, (uint32_t)groups);
    NVO_CHECK_LAUNCH();
    return NVO_OK;
}

int nvo_lattice_positions(nvo_stream_t stream, const nvo_lattice_args* args) {
    NVO_REQUIRE(args != nullptr, "lattice_positions: args is NULL");
    const nvo_lattice_args a = *args;
    NVO_REQUIRE(a.nx >= 1 && a.ny >= 1 && a.nz >= 1 && (uint64_t)a.nx * a.ny < (1ull << 32), "lattice_positions: bad lattice %u x %u x %u",
                a.nx, a.ny, a.nz);
    NVO_REQUIRE(a.first + a.count <= (uint64_t)a.nx * a.ny * a.nz, "lattice_positions: points %llu .. +%u lie outside the lattice",
                (unsigned long long)a.first, a.count);
    if (a.count == 0) return NVO_OK;
    NVO_REQUIRE(a.positions != nullptr, "lattice_positions: NULL positions");
    NVO_PROF(stream, "lattice_positions");
    NVO_LAUNCH(k_lattice_positions, dim3(nvo_div_up(a.count, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, a);
    NVO_CHECK_LAUNCH();
    return NVO_OK;
}

}  // extern "C"
