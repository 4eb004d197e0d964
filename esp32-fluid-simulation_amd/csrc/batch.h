// batch.h -- launch interface of the batched one-workgroup kernels (batch_grid.hip; internal, the public boundary is
// include/sfl.h sfl_batch_*).  A batch is B independent whole-domain grids of one shape that passes small_grid_fits (or
// large_member_fits: the launchers of batch_large.hip at the end of this file),
// stored member-major: member m of a field starts at element m * dim_x * dim_y.  Workgroup m steps / solves member m;
// members never communicate.  Every launcher is asynchronous on the given stream and returns the hipError_t of the launch.
#pragma once
#include "kernels.h"

struct sfl_open_flux;   // include/sfl.h

namespace sfl {

// One step (ino:252-287) of every member.  `step` describes member 0: its arrays (the kernel adds each member's offset,
// computed in 64-bit), the shape and the parameters, which every member shares.  Forces: force_offsets == nullptr = none;
// else B + 1 ints, and member m applies records [force_offsets[m], force_offsets[m + 1]) of step.force_cells /
// step.force_vel in that order (step.n_forces is ignored).
struct BatchStep {
    SmallStep step;
    const int *force_offsets;
};
hipError_t launch_batch_step(hipStream_t s, const BatchStep &a, int batch);
// poisson_solve (poisson.cpp:114-125) of every member: p = iters red-black SOR iterations from zero on rhs d.
hipError_t launch_batch_solve(hipStream_t s, float *p, const float *d, int dim_x, int dim_y, int batch, int iters,
                              SorParams prm);


// ---- per-member parameters ----------------------------------------------------------------------------------------
// What the two kernels above take once for all members, for ONE member, with the host-derived constants already formed
// (batch.cpp: by the expressions of the uniform path), and which member that is.  36 bytes; workgroup k of a launch
// runs record k of a device array that holds every member exactly once, in any order (batch.cpp: most iterations first).
struct BatchMember {
    float dt, two_dx_inv;
    SorParams prm;
    int iters;
    int member;
};
// launch_batch_step / launch_batch_solve with the dt, two_dx_inv, iters and prm of member m = members[k].member taken
// from members[k] (those of `step` are ignored), and report[m] = member m's update norm (include/sfl.h sfl_batch_residual): max over all cells of
// |p_gs - p| on the pressure the call leaves, a NaN if any term is one.  members and report: device arrays of `batch`.
hipError_t launch_batch_step_each(hipStream_t s, const BatchStep &a, int batch, const BatchMember *members, float *report);
hipError_t launch_batch_solve_each(hipStream_t s, float *p, const float *d, int dim_x, int dim_y, int batch,
                                   const BatchMember *members, float *report);

// ---- per-member parameters, the solve stopped at a tolerance ------------------------------------------------------
// sfl_member_stop of the member that members[k] names: stops[k] goes with members[k] (a device array of its own, so that
// BatchMember and the *_each kernels that read it stay as they are).  members[k].iters is the cap.
struct BatchStop {
    float tol;
    int every;
};
// launch_batch_step_each / launch_batch_solve_each with every solve run by the rule of include/sfl.h (sfl_member_stop):
// report[m] = the update norm of the pressure member m is left with, counts[2 m] = the iterations its solve ran,
// counts[2 m + 1] = that count again (solve; step with add == false) or added to what is there (step with add == true:
// the later steps of one call).  stops, report, counts: device arrays of `batch`, `batch` and 2 * `batch`.
hipError_t launch_batch_step_until(hipStream_t s, const BatchStep &a, int batch, const BatchMember *members,
                                   const BatchStop *stops, float *report, int *counts, bool add);
hipError_t launch_batch_solve_until(hipStream_t s, float *p, const float *d, int dim_x, int dim_y, int batch,
                                    const BatchMember *members, const BatchStop *stops, float *report, int *counts);

// ---- large members: up to kLargeMemberMaxCells cells, 8 B of LDS per cell (batch_large.hip, large_member_core.h) ----
// The same six launches for the batches of sfl_batch_create_large: one workgroup of 1024 threads per member whose LDS
// holds the advected velocity first and the divergence and the pressure afterwards (DESIGN.md has the layout and its
// barriers).  Same arguments, same results bit for bit; any shape that passes large_member_fits, however small.
constexpr int kLargeMemberMaxCells = 20224;    // (163840 - 2048) / 8: SFL_BATCH_LARGE_MAX_CELLS of include/sfl.h
constexpr int kLargeMemberMaxColour = 10240;   // cells of one colour: ten positions per thread and colour at 1024 threads
inline bool large_member_fits(int dim_x, int dim_y)
{
    return dim_x >= 2 && dim_y >= 2 && (long long)dim_x * dim_y <= kLargeMemberMaxCells &&
           (long long)dim_y * ((dim_x + 1) / 2) <= kLargeMemberMaxColour;
}
hipError_t launch_batch_large_step(hipStream_t s, const BatchStep &a, int batch);
hipError_t launch_batch_large_solve(hipStream_t s, float *p, const float *d, int dim_x, int dim_y, int batch, int iters,
                                    SorParams prm);
hipError_t launch_batch_large_step_each(hipStream_t s, const BatchStep &a, int batch, const BatchMember *members,
                                        float *report);
hipError_t launch_batch_large_solve_each(hipStream_t s, float *p, const float *d, int dim_x, int dim_y, int batch,
                                         const BatchMember *members, float *report);
hipError_t launch_batch_large_step_until(hipStream_t s, const BatchStep &a, int batch, const BatchMember *members,
                                         const BatchStop *stops, float *report, int *counts, bool add);
hipError_t launch_batch_large_solve_until(hipStream_t s, float *p, const float *d, int dim_x, int dim_y, int batch,
                                          const BatchMember *members, const BatchStop *stops, float *report, int *counts);

// ---- `steps` consecutive steps of every member in ONE launch (batch_play.hip) ---------------------------------------
// For the batches of sfl_batch_create (16 B of LDS per cell).  `step` describes member 0 as in BatchStep; the velocity is
// read from step.v_in before the first step and written to step.v_out, with step.div and step.p, after the last one; the
// dye ping-pongs between step.col_in and step.col_out inside the launch: step k reads col_in when k is even and col_out
// when it is odd, and writes the other, so the dye ends in col_out when `steps` is odd and in col_in when it is even.
// Forces: force_rows == nullptr = none; else row k, k in [0, rows), is the BatchStep::force_offsets of step k -- the
// `batch` + 1 ints at force_rows + k * batch, indices into step.force_cells / step.force_vel -- and steps k >= rows have
// none (rows <= steps).  members == nullptr: every member runs step's dt, two_dx_inv, iters and prm and nothing is
// reported; else records and report as for launch_batch_step_each, the update norm being that of the last step's solve.
// Every field ends up bit for bit where `steps` launches of launch_batch_step[_each] leave it.  steps >= 1.
struct BatchPlay {
    SmallStep step;
    const int *force_rows;
    int rows, steps;
};
hipError_t launch_batch_play(hipStream_t s, const BatchPlay &a, int batch, const BatchMember *members, float *report);

// ---- members with solid cells inside their grids (batch_solids.hip; include/sfl.h "SOLIDS") --------------------------
// One code byte per cell (advect_math.h: bits 0..3 W, E, S, N neighbour present, bit 4 the cell is fluid, a solid cell's
// byte 0), member-major like the fields: member m's bytes start at codes + m * member_stride, member_stride = dim_x * dim_y,
// or 0 for one mask that all members share.  Formed by the host from the user's mask (solids.cpp), consistent with the
// shape: a set neighbour bit never points outside the member.
struct BatchSolids {
    const uint8_t *codes;
    size_t member_stride;
};
// launch_batch_step[_each] and launch_batch_solve[_each] by the rule of include/sfl.h "SOLIDS", for the batches of
// sfl_batch_create (16 B of LDS per cell); report[m] = the update norm over member m's FLUID cells.  Same arguments
// otherwise; with no solid cell in a member, the same results bit for bit.
hipError_t launch_batch_solid_step(hipStream_t s, const BatchStep &a, const BatchSolids &solids, int batch);
hipError_t launch_batch_solid_step_each(hipStream_t s, const BatchStep &a, const BatchSolids &solids, int batch,
                                        const BatchMember *members, float *report);
hipError_t launch_batch_solid_solve(hipStream_t s, float *p, const float *d, const BatchSolids &solids, int dim_x, int dim_y,
                                    int batch, int iters, SorParams prm);
hipError_t launch_batch_solid_solve_each(hipStream_t s, float *p, const float *d, const BatchSolids &solids, int dim_x, int dim_y,
                                         int batch, const BatchMember *members, float *report);
// The velocity part of launch_flow_stats (stats_kernels.h) with the divergence of the rule's item 4: atomic maxima into
// out[m], which the caller has zeroed on the stream in front.
struct FlowStatsRecord;
hipError_t launch_solid_velocity_stats(hipStream_t s, FlowStatsRecord *out, const float *v, const BatchSolids &solids, int dim_x,
                                       int dim_y, int members, float two_dx_inv, const float *member_two_dx_inv);

// ---- members with openings on the rim of their grids (batch_openings.hip; include/sfl.h "OPENINGS") ------------------
// One OPEN CODE of 16 bits per cell (advect_math.h: the code byte of the solids in bits 0..7, which neighbour is open in
// bits 8..11, bit 12 = outflow), member-major: member m's start at codes + m * member_stride, member_stride = dim_x * dim_y
// or 0 for codes that all members share.  An array of its own, formed by the host (openings.cpp): the code bytes that the
// solids', loads' and viscous kernels read are not touched.  inflow: member m's (x, y) at inflow + 2 * m.
struct BatchOpenings {
    const uint16_t *codes;
    size_t member_stride;
    const float *inflow;
};
// launch_batch_solid_step[_each], _solve[_each] and launch_solid_velocity_stats by the rule of "OPENINGS"; with no opening
// in a member, the same results bit for bit.
hipError_t launch_batch_open_step(hipStream_t s, const BatchStep &a, const BatchOpenings &open, int batch);
hipError_t launch_batch_open_step_each(hipStream_t s, const BatchStep &a, const BatchOpenings &open, int batch,
                                       const BatchMember *members, float *report);
hipError_t launch_batch_open_solve(hipStream_t s, float *p, const float *d, const BatchOpenings &open, int dim_x, int dim_y,
                                   int batch, int iters, SorParams prm);
hipError_t launch_batch_open_solve_each(hipStream_t s, float *p, const float *d, const BatchOpenings &open, int dim_x, int dim_y,
                                        int batch, const BatchMember *members, float *report);
hipError_t launch_open_velocity_stats(hipStream_t s, FlowStatsRecord *out, const float *v, const BatchOpenings &open, int dim_x,
                                      int dim_y, int members, float two_dx_inv, const float *member_two_dx_inv);

// ---- members with an inflow profile, and the flux through the openings (include/sfl.h "INFLOW PROFILES AND FLUX") ----
// The profile as ONE CSR table on the device, formed by the host (inflow.cpp) once per change of the profile, the map or
// the mask: member m's records are [offsets[m], offsets[m + 1]), record k the cell index cells[k] -- a FLUID inflow cell
// of that member, unique within the row -- and its velocity (vel[2 * k], vel[2 * k + 1]).
struct BatchProfile {
    const int *offsets;
    const uint32_t *cells;
    const float *vel;
};
// launch_batch_open_step[_each] (batch_openings.hip) with the records of the member's row written behind the advection:
// with empty rows, or rows that hold the uniform inflow, the same results bit for bit.
hipError_t launch_batch_open_profile_step(hipStream_t s, const BatchStep &a, const BatchOpenings &open, const BatchProfile &profile, int batch);
hipError_t launch_batch_open_profile_step_each(hipStream_t s, const BatchStep &a, const BatchOpenings &open, const BatchProfile &profile,
                                               int batch, const BatchMember *members, float *report);
// out[k] = the flux record of member first + k, k in [0, count), from the velocity at v (member 0's) and the open codes
// (inflow.hip): one launch, one workgroup per member, ordinary stores.
hipError_t launch_batch_open_flux(hipStream_t s, struct sfl_open_flux *out, const float *v, const BatchOpenings &open, int dim_x, int dim_y,
                                  int first, int count);

// ---- members whose solid cells move (batch_walls.hip; include/sfl.h "WALL VELOCITIES") -------------------------------
// The wall table is a BatchProfile: member m's records are [offsets[m], offsets[m + 1]), record k the cell index cells[k]
// -- a SOLID cell of that member, unique within the row, in cell order -- and its velocity.  Formed by the host
// (walls.cpp, wall_table.h) once per sfl_batch_set_wall_velocity.  Two pairs of kernels:
//   * on the solids' bytes: launch_batch_viscous_solid_step[_each] with the row; visc == nullptr = no member has item 3a
//     (launch_batch_solid_step[_each] with the row);
//   * on open codes: launch_batch_open_profile_step[_each] with the row; profile.offsets == nullptr = no profile
//     (launch_batch_open_step[_each] with the row).
// With empty rows, or rows of +0.0f, the same results bit for bit as those launches.
struct BatchViscous;   // viscous_kernels.h
hipError_t launch_batch_wall_step(hipStream_t s, const BatchStep &a, const BatchSolids &solids, const BatchViscous *visc,
                                  const BatchProfile &walls, int batch);
hipError_t launch_batch_wall_step_each(hipStream_t s, const BatchStep &a, const BatchSolids &solids, const BatchViscous *visc,
                                       const BatchProfile &walls, int batch, const BatchMember *members, float *report);
hipError_t launch_batch_open_wall_step(hipStream_t s, const BatchStep &a, const BatchOpenings &open, const BatchProfile &profile,
                                       const BatchProfile &walls, int batch);
hipError_t launch_batch_open_wall_step_each(hipStream_t s, const BatchStep &a, const BatchOpenings &open, const BatchProfile &profile,
                                            const BatchProfile &walls, int batch, const BatchMember *members, float *report);

// ---- the draw task of many members in one launch (batch_render.hip) -----------------------------------------------
// Image k of `images` (k in [0, count), member-major: image k starts at pixel k * H * W, H = scaling * (dim_x - 1) rows of
// W = scaling * (dim_y - 1) uint16) = launch_render_rgb565 of the dye at colour_of_first_member + 3 * k * dim_x * dim_y,
// bit for bit.  Member bases are formed in 64-bit, offsets inside one member in 32-bit (H * W <= 2^31 - 1: the caller's
// limits on cells and scaling see to it).  Either kind of batch; scaling >= 1; count == 0 launches nothing.
hipError_t launch_batch_render(hipStream_t s, uint16_t *images, const uint32_t *colour_of_first_member, int dim_x, int dim_y,
                               int count, int scaling, bool byteswap);

}  // namespace sfl
