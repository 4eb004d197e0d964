// view_kernels.h -- launch interface of the kernels behind sfl_view_* / sfl_batch_view_* (field_view.hip); internal, as
// kernels.h, whose types it uses.  Called from views.cpp only.  Every launcher is asynchronous on the given stream and
// returns the hipError_t of its launch.  A context is a batch of one member.
#pragma once
#include "kernels.h"

namespace sfl {

constexpr int kViewMaxStops = 256;                          // stops of a palette (include/sfl.h, struct sfl_view)
constexpr int kViewPaletteWords = 3 + 3 * kViewMaxStops;    // words of the largest staged palette

// The fields the views of `count` members are derived from: member k's velocity at v + 2 * k * dim_x * dim_y (8-byte
// aligned), its pressure at p + k * dim_x * dim_y; bases are formed in 64-bit.  Read only.
struct ViewFields {
    const float *v, *p;
    int dim_x, dim_y, count;
};

// struct sfl_view with the host-derived constants formed (views.cpp: two_dx_inv = 1.0f / (2.0f * dx) as the divergence
// forms it, r = 1.0f / (hi - lo)) and the palette in device memory: words 0..2 nan_colour, word 3 + 3 * n + k channel k of
// stop n, raw UQ32.  The scalar kernel reads `what` and `two_dx_inv` only.
struct ViewParams {
    int what;
    float two_dx_inv, lo, r;
    int stops;
    const uint32_t *palette;
};

// out[k * dim_x * dim_y + dim_x * j + i] = scalar `what` of member k at node (i, j) (include/sfl.h, "the four scalars").
hipError_t launch_view_scalar(hipStream_t s, float *out, const ViewFields &f, int what, float two_dx_inv);
// out[3 * (k * dim_x * dim_y + dim_x * j + i) + c] = channel c of that node's texel: the scalar through the palette.
hipError_t launch_view_texels(hipStream_t s, uint32_t *out, const ViewFields &f, const ViewParams &v);
// Image k of `images` (member-major, as launch_batch_render lays them out) = launch_batch_render of a member whose dye is
// member k's texels, bit for bit.  Offsets inside one image are 32-bit: H * W <= 2^31 - 1 is the caller's to check.
hipError_t launch_view_render(hipStream_t s, uint16_t *images, const ViewFields &f, const ViewParams &v, int scaling,
                              bool byteswap);

}  // namespace sfl
