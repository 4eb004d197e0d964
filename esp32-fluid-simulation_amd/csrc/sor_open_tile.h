// sor_open_tile.h -- the tile of sor_solid_tile.h for a context with openings (include/sfl.h "OPENINGS", item 5): the load,
// the half-sweeps and the store are that tile's, unchanged; behind the load the k of a cell whose open neighbour is an
// OUTFLOW is set up from n = present + 1 -- the outflow's ghost pressure of zero counts as a neighbour, contributes -0.0f to the
// sum as an absent one does and leaves z at +0.0f.  One OPEN BYTE per cell beside the code byte: bits 0..3 say which neighbour
// (W, E, S, N: the one outside the domain) is open, bit 4 that it is an outflow; 0 in a cell that is solid or has no opening.
// Host and device, as the tile is: the host's emulation of a launch runs the same statements.
#pragma once
#include "sor_solid_tile.h"

namespace sfl {
namespace open_tile {

constexpr int kOpenSides = 15, kOpenOutflow = 16;

// n of item 5: the present neighbours, and one more for an outflow
SFL_HD int neighbours_of(int code, int open) { return solid_tile::present_of(code) + ((open & kOpenOutflow) ? 1 : 0); }

// An opening lies on the rim of the domain: a tile whose window -- the cells a launch relaxes -- does not reach the rim has no
// outflow cell and skips the set-up below whole.  The same for every thread of a workgroup.
SFL_HD bool window_reaches_rim(const solid_tile::Tile &t)
{
    using namespace solid_tile;
    return t.x0 - kHalo <= 0 || t.y0 - kHalo <= 0 || t.x0 + kTX + kHalo >= t.dim_x || t.y0 + kTY + kHalo >= t.dim_y;
}

// behind solid_tile::load: the k of the thread's outflow cells
SFL_HD void set_up_k(solid_tile::Cells &c, const solid_tile::Tile &t, const uint8_t *open, int tid)
{
    using namespace solid_tile;
    if (!window_reaches_rim(t)) return;
#pragma unroll
    for (int colour = 0; colour < 2; ++colour)
#pragma unroll
        for (int s = 0; s < kSlots; ++s) {
            const int code = c.code[colour][s];
            if (!code) continue;   // (not relaxed: outside, on the ring, or solid)
            const Spot o = spot_of(tid, colour, s);
            const int gx = t.x0 - kHalo + o.wi, gy = t.y0 - kHalo + o.wj;
            const int op = open[(size_t)gy * (size_t)t.dim_x + (size_t)gx];
            if (op & kOpenOutflow) c.kf[colour][s] = k_factor(neighbours_of(code, op));
        }
}

}  // namespace open_tile
}  // namespace sfl
