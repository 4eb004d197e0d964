// until_kernels.h -- launch interface of the kernels behind sfl_residual, sfl_poisson_continue and sfl_poisson_solve_until
// (internal, as kernels.h, whose types it uses): the update norm of a field of any size (update_norm.hip) and the two
// one-workgroup solves of small_grid.hip that start from a pressure or stop at a tolerance.  Called from solve_until.cpp
// alone.  Every launcher is asynchronous on the given stream and returns the hipError_t of the launch.
#pragma once
#include "kernels.h"

namespace sfl {

// ---- the update norm (update_norm.hip) ------------------------------------------------------------------
// *worst (a device word, zeroed here on the stream in front of the kernel) = the bits of max |p_gs(c) - p(c)| over the
// cells of global rows [g_begin, g_end): include/sfl.h sfl_residual.  A float maximum when no cell's is a NaN, else a NaN.
// One streaming pass over p and d at any dim_x >= 2 and any alignment.  Needs p on rows [g_begin - 1, g_end + 1) clipped to
// the domain (a slab: one exact ghost row beside each cut).
hipError_t launch_update_norm(hipStream_t s, unsigned *worst, const float *p, const float *d, Slab g, int g_begin,
                              int g_end, float dx);

// ---- small grids (small_grid.hip; the shapes of small_grid_fits) ------------------------------------------
// `iters` MORE iterations on the pressure p holds (sfl_poisson_continue): the same cells, passes and expressions as
// launch_small_solve, started from p instead of zero; in place, one launch.
hipError_t launch_small_solve_warm(hipStream_t s, float *p, const float *d, int dim_x, int dim_y, int iters, SorParams prm);
// The solve from zero stopped by the rule of include/sfl.h sfl_member_stop (cap, tol, every), one launch: p = the pressure
// of the k iterations it ran, result[0] = the bits of the update norm u_k of that pressure, result[1] = k (device words).
hipError_t launch_small_solve_until(hipStream_t s, float *p, const float *d, int dim_x, int dim_y, int cap, SorParams prm,
                                    float tol, int every, unsigned *result);

}  // namespace sfl
