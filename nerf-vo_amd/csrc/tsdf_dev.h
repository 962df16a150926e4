// The per-voxel TSDF fusion rule (DESIGN.md "TSDF fusion") and the launchers' argument checks, shared by tsdf.hip (the
// dense volume) and tsdf_blocks.hip / iso_blocks.hip (the block-sparse one).  The rule exists here and nowhere else;
// tests/test_tsdf_bits_gpu.py pins the bits it produces in both volumes.
#pragma once
#include "nvo_common.h"
#include "../../include/nerfvo_hip.h"

#include <math.h>

// Apply the frames of `live` (bit f: frame f of the K in the LDS table `cam`, 16 floats each: world->camera 3x4, fx fy cx
// cy) in table order to the voxel at (px, py, pz):
//
//   (xc,yc,zc) = R p + t                                  skip if zc <= 0
//   u = fx*xc/zc + cx, v = fy*yc/zc + cy                  ui = floor(u + 0.5), vi = floor(v + 0.5); skip off-image
//   d = depth[f][vi][ui]                                  skip unless 0 < d <= depth_max;  sdf = d - zc; skip if < -trunc
//   s = min(sdf, trunc) / trunc                           tsdf = (w*tsdf + s)/(w+1), colour likewise, w += 1
//
// all in fp32 as written (the library is built with -ffp-contract=off).  The voxel's five values -- tsdf[idx],
// weight[idx] and color[cidx], color[cstride + cidx], color[2 cstride + cidx] -- live in registers across the frames,
// are loaded when the first frame touches them and stored once.  (The arrays and the voxel's indices, not pointers to
// the voxel's entries: with a launch-uniform cstride the compiler then keeps the bases of the three colour planes in
// scalar registers, as k_tsdf_integrate had them.)
static __device__ __forceinline__ void tsdf_fuse_voxel(const float* cam, uint32_t K, uint32_t live, uint32_t H, uint32_t W, float fW,
                                                       float fH, const float* depth, const uint8_t* rgb, float trunc, float depth_max,
                                                       float px, float py, float pz, float* tsdf, float* weight, float* color,
                                                       size_t idx, size_t cidx, size_t cstride) {
    bool touched = false;
    float t = 0.f, w = 0.f, cr = 0.f, cg = 0.f, cb = 0.f;
    for (uint32_t f = 0; f < K; ++f) {
        if (!((live >> f) & 1u)) continue;
        const float* c = cam + 16 * f;
        const float zc = c[8] * px + c[9] * py + c[10] * pz + c[11];
        if (zc <= 0.f) continue;
        const float xc = c[0] * px + c[1] * py + c[2] * pz + c[3];
        const float yc = c[4] * px + c[5] * py + c[6] * pz + c[7];
        const float u = c[12] * xc / zc + c[14], v = c[13] * yc / zc + c[15];
        const float ui = floorf(u + 0.5f), vi = floorf(v + 0.5f);
        if (!(ui >= 0.f && ui < fW && vi >= 0.f && vi < fH)) continue;  // a NaN fails
        const size_t pix = ((size_t)f * H + (uint32_t)vi) * W + (uint32_t)ui;
        const float d = depth[pix];
        if (!(d > 0.f && d <= depth_max)) continue;  // a NaN fails
        const float sdf = d - zc;
        if (sdf < -trunc) continue;
        if (!touched) {
            t = tsdf[idx];
            w = weight[idx];
            cr = color[cidx];
            cg = color[cstride + cidx];
            cb = color[2 * cstride + cidx];
            touched = true;
        }
        const float s = fminf(sdf, trunc) / trunc;
        const uint8_t* p = rgb + 3 * pix;
        const float w1 = w + 1.f;
        t = (w * t + s) / w1;
        cr = (w * cr + (float)p[0]) / w1;
        cg = (w * cg + (float)p[1]) / w1;
        cb = (w * cb + (float)p[2]) / w1;
        w = w1;
    }
    if (touched) {
        tsdf[idx] = t;
        weight[idx] = w;
        color[cidx] = cr;
        color[cstride + cidx] = cg;
        color[2 * cstride + cidx] = cb;
    }
}

// ---- host: what every launcher that takes a frame table or a block table requires of it ----
static inline int tsdf_frames_check(const char* what, uint32_t K, uint32_t H, uint32_t W, float voxel_size, float trunc) {
    NVO_REQUIRE(K >= 1 && K <= NVO_TSDF_MAX_FRAMES, "%s: %u frames per launch not in 1..%u", what, K, (uint32_t)NVO_TSDF_MAX_FRAMES);
    NVO_REQUIRE(H >= 1 && W >= 1 && H <= (1u << 16) && W <= (1u << 16), "%s: frame size %u x %u not in 1..65536", what, W, H);
    NVO_REQUIRE(voxel_size > 0.f && voxel_size < INFINITY && trunc > 0.f && trunc < INFINITY,
                "%s: voxel_size %g and trunc %g must be positive and finite", what, (double)voxel_size, (double)trunc);
    return NVO_OK;
}

static inline int tsdf_table_check(const char* what, uint32_t tbx, uint32_t tby, uint32_t tbz, uint64_t* n_table) {
    NVO_REQUIRE(tbx >= 1 && tby >= 1 && tbz >= 1 && tbx <= NVO_TSDF_BLOCKS_MAX_TABLE && tby <= NVO_TSDF_BLOCKS_MAX_TABLE &&
                    tbz <= NVO_TSDF_BLOCKS_MAX_TABLE && (uint64_t)tbx * tby <= NVO_TSDF_BLOCKS_MAX_TABLE &&
                    (uint64_t)tbx * tby * tbz <= NVO_TSDF_BLOCKS_MAX_TABLE,
                "%s: block table %u x %u x %u must have between 1 and 2^26 entries", what, tbx, tby, tbz);
    *n_table = (uint64_t)tbx * tby * tbz;
    return NVO_OK;
}
