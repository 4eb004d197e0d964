// viscous_kernels.h -- launch interface of the kernels behind the viscosity (internal, as batch.h, whose types it uses;
// include/sfl.h "VISCOSITY"): context_viscous.hip, called from context_viscous.cpp alone, and batch_viscous.hip, called
// from viscous.cpp alone.  Every launcher is asynchronous on the given stream and returns the hipError_t of its launch.
#pragma once
#include "batch.h"

namespace sfl {

// ---- whole-domain contexts (context_viscous.hip; diffuse_tile.h) -------------------------------------------------------
// ONE launch of the diffusion on WHOLE-DOMAIN arrays of dim_x x dim_y cells of two floats, any size: k sweeps,
// 1 <= k <= diffuse::kD, from u_in into u_out with u0 what items 1 to 3 left (the first launch of a diffusion: u_in
// itself).  u_out aliases neither.  Every cell of u_out is written.  codes: one byte per cell (solids.cpp solid_codes)
// or null without solids; zero_solids: a solid cell's velocity is read as (0, 0) and stored so (item 3 inside a step).
hipError_t launch_diffuse_velocity(hipStream_t s, float *u_out, const float *u_in, const float *u0, const uint8_t *codes,
                                   int dim_x, int dim_y, int k, float a, float c, bool zero_solids);

// ---- batch members (batch_viscous.hip) ----------------------------------------------------------------------------------
// Item 3a of ONE member, with the host-derived constants already formed (viscous.cpp: diffuse::coefficients of that
// member's nu, dt and dx).  sweeps == 0: the member skips the item whole (the host stores 0 for nu == 0 too).  12 bytes;
// a device array of `batch`, record m member m's whatever the launch order -- a table of its own: BatchMember and the
// kernels that read it stay as they are.
struct BatchViscous {
    float a, c;
    int sweeps;
};
// launch_batch_step[_each] (batch.h) with item 3a between the forces and the divergence, and launch_batch_solid_step[_each]
// with it between items 3 and 4, for the batches of sfl_batch_create (16 B of LDS per cell and not a byte more: u0 lives
// where d and p will).  Same arguments otherwise; with sweeps == 0 in every record the same results bit for bit.
hipError_t launch_batch_viscous_step(hipStream_t s, const BatchStep &a, const BatchViscous *visc, int batch);
hipError_t launch_batch_viscous_step_each(hipStream_t s, const BatchStep &a, const BatchViscous *visc, int batch,
                                          const BatchMember *members, float *report);
hipError_t launch_batch_viscous_solid_step(hipStream_t s, const BatchStep &a, const BatchSolids &solids, const BatchViscous *visc,
                                           int batch);
hipError_t launch_batch_viscous_solid_step_each(hipStream_t s, const BatchStep &a, const BatchSolids &solids,
                                                const BatchViscous *visc, int batch, const BatchMember *members, float *report);

}  // namespace sfl
