// solid_kernels.h -- launch interface of the kernels behind the solid cells of a whole-domain context (internal, as
// kernels.h, whose types it uses; include/sfl.h "SOLIDS OF A CONTEXT"): context_solids.hip.  Called from
// context_solids.cpp alone.  WHOLE-DOMAIN arrays of dim_x x dim_y cells of any size; `codes` is one byte per cell
// (solids.cpp solid_codes).  Every launcher is asynchronous on the given stream and returns the hipError_t of its
// launches.
#pragma once
#include "kernels.h"

namespace sfl {

// Item 4 of the rule: div = the divergence of every fluid cell, 0.0f in a solid one; a neighbour that is not present is
// never read.  zero_solids (inside a step, item 3): the velocity of every solid cell is also set to (0, 0) -- no fluid
// cell reads it, so the one pass does both.
hipError_t launch_solid_divergence(hipStream_t s, float *div, float *v, const uint8_t *codes, int dim_x, int dim_y,
                                   float two_dx_inv, bool zero_solids);

// Item 6: v -= grad p with an absent neighbour's pressure the cell's own; (0, 0) into solid cells.  In place.
hipError_t launch_solid_gradient(hipStream_t s, float *v, const float *p, const uint8_t *codes, int dim_x, int dim_y,
                                 float two_dx_inv);

// ONE launch of the masked solve (sor_solid_tile.h): k iterations, 1 <= k <= solid_tile::kD, from p_in (null: from zero
// everywhere) into p_out, which must not alias p_in.  Every cell of p_out is written.
hipError_t launch_solid_sor(hipStream_t s, float *p_out, const float *p_in, const float *d, const uint8_t *codes, int dim_x,
                            int dim_y, int k, SorParams prm);

// *worst (a device word, zeroed here on the stream in front) = the bits of the maximum over the FLUID cells of
// |p_gs - p| on the pressure as it stands; 0 without a fluid cell; any NaN wins.
hipError_t launch_solid_update_norm(hipStream_t s, unsigned *worst, const float *p, const float *d, const uint8_t *codes,
                                    int dim_x, int dim_y, float dx);

// *worst (zeroed here in front) = the bits of the maximum of |divergence by item 4| over all cells.
hipError_t launch_solid_max_divergence(hipStream_t s, unsigned *worst, const float *v, const uint8_t *codes, int dim_x,
                                       int dim_y, float two_dx_inv);

}  // namespace sfl
