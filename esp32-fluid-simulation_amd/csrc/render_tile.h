// render_tile.h -- the tile scheme of the LDS-staged draw, shared by the two kernels that use it: batch_render.hip (the
// load phase copies the dye's texels) and field_view.hip (the load phase derives the texels from the velocity or the
// pressure).  One workgroup of kThreads draws one tile of kTileI x kTileJ cell blocks of one member from the tile's
// (kTileI + 1) x (kTileJ + 1) corner texels, which its load phase has left in LDS, widened to float: word 3 * it + k of
// column jt at jt * kPitch.  batch_render.hip has the layout's bank argument; the arithmetic is render_math.h's.
#pragma once
#include "render_math.h"

namespace sfl {
namespace render_tile {

constexpr int kThreads = 256;
constexpr int kTileI = 16, kTileJ = 32;         // cell blocks per tile, down (i) and across (j) the screen
constexpr int kPitch = 3 * (kTileI + 1);        // words per staged column: odd (batch_render.hip)
constexpr int kTexelWords = (kTileJ + 1) * kPitch;
// workgroups of a launch; they stride over the (member, tile) pairs.  32 per CU of the device's 256: every pair costs
// the same, so more would balance nothing, and a batch of more than 65536 members takes the loop's later passes
constexpr unsigned kMaxGrid = 1u << 16;
static_assert(kPitch % 2 == 1, "an odd pitch keeps 32 consecutive columns on 32 banks");

// draw: rows * scaling image rows of cols blocks of the tile at block (i0, j0); one thread takes the `scaling` pixels of
// one block in one image row: both edge walks once, then ONE walk across (pixel jj + 1 continues the chain of pixel jj).
// `image`: the member's first pixel, `width` pixels per image row.  The caller's barriers stand around it.
__device__ __forceinline__ void draw_tile(const float *texel, uint16_t *image, int i0, int j0, int rows, int cols, int scaling,
                                          int width, float inv, int byteswap)
{
    using namespace render_math;
    for (int n = threadIdx.x; n < rows * scaling * cols; n += kThreads) {
        const int py = n / cols, jt = n - py * cols;
        const int it = py / scaling, ii = py - it * scaling;
        const float *t1 = texel + jt * kPitch + 3 * it, *t2 = t1 + kPitch;
        RenderWalk red(render_walk(t1[0], t1[3], inv, ii), render_walk(t2[0], t2[3], inv, ii), inv);
        RenderWalk green(render_walk(t1[1], t1[4], inv, ii), render_walk(t2[1], t2[4], inv, ii), inv);
        RenderWalk blue(render_walk(t1[2], t1[5], inv, ii), render_walk(t2[2], t2[5], inv, ii), inv);
        const auto next = [&]() {
            const uint16_t px = render_pack(advect_math::uq_narrow(red.x), advect_math::uq_narrow(green.x),
                                            advect_math::uq_narrow(blue.x), byteswap);
            red.step();
            green.step();
            blue.step();
            return px;
        };
        uint16_t *out = image + ((i0 * scaling + py) * width + (j0 + jt) * scaling);
        // pairs of pixels as one 32-bit store where this thread's pixels allow it: an even count on a 4-byte boundary
        // (a member's image starts on a 2-byte boundary only)
        if ((scaling & 1) == 0 && (reinterpret_cast<uintptr_t>(out) & 3) == 0) {
            for (int jj = 0; jj < scaling; jj += 2) {
                const uint32_t lo = next(), hi = next();
                *reinterpret_cast<uint32_t *>(out + jj) = lo | (hi << 16);
            }
        } else {
            for (int jj = 0; jj < scaling; ++jj) out[jj] = next();
        }
    }
}

}  // namespace render_tile
}  // namespace sfl
