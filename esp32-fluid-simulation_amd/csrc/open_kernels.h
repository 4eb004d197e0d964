// open_kernels.h -- launch interface of context_openings.hip (and of the context's two launches of inflow.hip): the kernels of a whole-domain context with openings (include/sfl.h
// "OPENINGS OF A CONTEXT").  codes: the code byte of every cell (advect_math.h; all fluid where no mask is set); open: the open
// byte of every cell (sor_open_tile.h).  Otherwise the arguments and the results of solid_kernels.h.
#pragma once
#include "kernels.h"

struct sfl_open_flux;   // include/sfl.h

namespace sfl {

// v[cells[k]] = inflow for the n cells of the compact list (item 2a)
hipError_t launch_open_inflow(hipStream_t s, float *v, const uint32_t *cells, int n, float inflow_x, float inflow_y);
// ... with a profile (inflow.hip): v[cells[k]] = (values[2 * k], values[2 * k + 1])
hipError_t launch_open_inflow_profile(hipStream_t s, float *v, const uint32_t *cells, const float *values, int n);
// the flux record of the velocity at v through the live open cells (inflow.hip): one workgroup over the rim, ordinary stores
hipError_t launch_open_flux(hipStream_t s, struct sfl_open_flux *out, const float *v, const uint8_t *open, int dim_x, int dim_y);
hipError_t launch_open_divergence(hipStream_t s, float *div, float *v, const uint8_t *codes, const uint8_t *open, int dim_x, int dim_y,
                                  float two_dx_inv, bool zero_solids);
hipError_t launch_open_gradient(hipStream_t s, float *v, const float *p, const uint8_t *codes, const uint8_t *open, int dim_x, int dim_y,
                                float two_dx_inv);
hipError_t launch_open_sor(hipStream_t s, float *p_out, const float *p_in, const float *d, const uint8_t *codes, const uint8_t *open,
                           int dim_x, int dim_y, int k, SorParams prm);
hipError_t launch_open_update_norm(hipStream_t s, unsigned *worst, const float *p, const float *d, const uint8_t *codes,
                                   const uint8_t *open, int dim_x, int dim_y, float dx);
hipError_t launch_open_max_divergence(hipStream_t s, unsigned *worst, const float *v, const uint8_t *codes, const uint8_t *open,
                                      int dim_x, int dim_y, float two_dx_inv);

}  // namespace sfl
