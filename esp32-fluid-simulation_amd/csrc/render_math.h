// render_math.h -- per-pixel arithmetic of the dye visualiser (draw task, ino:116-176), written ONCE and
// shared by the one-thread-per-pixel kernel of a context (stencil_kernels.hip render_rgb565_kernel) and the LDS-staged
// kernel of a batch (batch_render.hip).
//
// Pixel (sy, sx) of an image at scaling S belongs to cell block (i, j) = (sy / S, sx / S) at offset (ii, jj).  It replays
// the sketch's strength-reduced lerps for its own offsets only: the left and the right edge after ii increments
// (:134-153), then jj increments across (:156-161), the narrowing to UQ32 (:168), the RGB565 pack (:170-172) and the
// optional byte swap (:173).  Compiled with -ffp-contract=off: every product and sum is rounded on its own, and a sum of
// n increments is n sequential additions, never n * d.
#pragma once
#include "advect_math.h"

namespace sfl {
namespace render_math {

// 1 / S as the sketch forms it
__device__ __forceinline__ float render_inv(int scaling) { return 1.0f / (float)scaling; }

// one lerp of the draw task, step by step: from `a` towards `b` in steps of (b - a) * inv added one after the other.  The
// value after n steps does not depend on who took the first n - 1: a thread that needs the values after 0, 1, 2 ... steps
// (the pixels of one block along an image row) takes them from one walk
struct RenderWalk {
    float x, d;
    __device__ __forceinline__ RenderWalk(float a, float b, float inv) : x(a), d((b - a) * inv) {}
    __device__ __forceinline__ void step() { x += d; }
};

// ... and its value after `n` steps (down an edge: a, b = the texels above and below, n = ii; across: a, b = the two
// edge values, n = jj)
__device__ __forceinline__ float render_walk(float a, float b, float inv, int n)
{
    RenderWalk w(a, b, inv);
    for (int k = 0; k < n; ++k) w.step();
    return w.x;
}

// one channel of one pixel from the four widened corner texels of its cell block: t11 = (i, j), t21 = (i + 1, j),
// t12 = (i, j + 1), t22 = (i + 1, j + 1)
__device__ __forceinline__ uint32_t render_channel(float t11, float t21, float t12, float t22, float inv, int ii, int jj)
{
    const float l = render_walk(t11, t21, inv, ii);
    const float r = render_walk(t12, t22, inv, ii);
    return advect_math::uq_narrow(render_walk(l, r, inv, jj));
}

// RGB565 of three UQ32 channels (their top 5, 6 and 5 bits), byte-swapped for a big-endian panel if asked
__device__ __forceinline__ uint16_t render_pack(uint32_t r, uint32_t g, uint32_t b, int byteswap)
{
    uint16_t px = (uint16_t)(((r & 0xF8000000u) >> 16) | ((g & 0xFC000000u) >> 21) | ((b & 0xF8000000u) >> 27));
    if (byteswap) px = (uint16_t)((px >> 8) | (px << 8));
    return px;
}

}  // namespace render_math
}  // namespace sfl
