// context_viscous.cpp -- viscosity of a whole-domain context (include/sfl.h "VISCOSITY"; sfl_set_viscosity, _viscosity_info,
// sfl_diffuse_velocity): the launches of context_viscous.hip that item 3a makes, and the unfused sequence a step runs
// while a viscosity is set.  Host C++ only.
//
// The step and the transports live in units that the host test harnesses link without this one, so they do not call into
// it: what a context holds of its viscosity is plain data on the struct (context.h ContextViscosity; sfl_destroy frees
// the third buffer), and the sequence is reached through its pointer, set here while a viscosity is set and null
// otherwise -- then a call launches exactly what it launched before there was viscosity.
#include "context.h"
#include "diffuse_tile.h"
#include "viscous_kernels.h"

#include <cmath>

using namespace sfl::host;

namespace {

// the checks every call makes on its numbers, in front of the handle's
int check_numbers(const char *call, float nu, int sweeps)
{
    if (std::isnan(nu) || nu < 0.0f) return fail(SFL_ERR_INVALID, "%s: nu must be >= 0 and not a NaN (got %g)", call, (double)nu);
    if (sweeps < 0) return fail(SFL_ERR_INVALID, "%s: sweeps must be >= 0 (got %d)", call, sweeps);
    return SFL_OK;
}

int check_whole_domain(const sfl_context *c, const char *call, const char *nothing)
{
    if (c->nranks != 1)
        return fail(SFL_ERR_STATE, "%s: whole-domain contexts only (slab %d/%d): a slab's exchanges do not know the diffusion's halo; %s", call,
                    c->rank, c->nranks, nothing);
    if (c->transport)
        return fail(SFL_ERR_STATE, "%s: the context has a transport attached, whose exchanges do not know the diffusion's halo: %s", call, nothing);
    return SFL_OK;
}

// Item 3a on the velocity held: ceil(sweeps / kD) launches.  The first reads the velocity as u and as u0 and writes
// vel_tmp; the later ones go between vel_tmp and the third buffer while the velocity, untouched, stays u0; the host then
// makes the buffer the last launch wrote the velocity.  sweeps <= kD allocate nothing beyond vel_tmp, which every step has.
int diffuse(sfl_context *c, float nu, float dt, float dx, int sweeps, bool zero_solids)
{
    namespace df = sfl::diffuse;
    if (nu == 0.0f || sweeps == 0) return SFL_OK;   // skipped whole: no bit changes
    SFL_TRY(ensure_field(c, SFL_FIELD_VELOCITY));
    SFL_TRY(ensure(c, c->vel_tmp, 8, false));
    if (sweeps > df::kD) SFL_TRY(ensure(c, c->viscosity.d_third, 8, false));   // (a failed allocation: SFL_ERR_NOMEM)
    SFL_TRY(use_device(c));
    const df::Coefficients k = df::coefficients(nu, dt, dx);
    const uint8_t *codes = c->solids.set ? c->solids.d_codes : nullptr;
    const float *in = c->vel;
    float *out = c->vel_tmp, *spare = c->viscosity.d_third;
    for (int l = 0; l < df::launches_of(sweeps); ++l) {
        HIP_TRY(sfl::launch_diffuse_velocity(c->stream, out, in, c->vel, codes, c->dim_x, c->gdim_y, df::sweeps_of_launch(sweeps, l), k.a, k.c,
                                             zero_solids && codes));
        in = out;
        std::swap(out, spare);   // (one launch: `spare` may be null and is never used)
    }
    // `in` holds the result: it becomes the velocity, and the velocity's buffer takes its place
    if (in == c->vel_tmp)
        std::swap(c->vel, c->vel_tmp);
    else
        std::swap(c->vel, c->viscosity.d_third);
    ++c->vel_epoch;
    c->v_ghost_valid = 0;
    return SFL_OK;
}

// One step with item 3a, behind sfl_step's checks: one unfused sequence -- the existing velocity advection, the existing
// forces, the diffusion (with solids: its first launch also zeroes the solid cells' velocity, item 3), then the
// divergence, the solve, the gradient and the dye advection as the calls of their own run them, by the solids' rule
// where a mask is set.  No seam, no fused kernel, no small-grid one-launch step.
// (context_walls.cpp's step restates this sequence with one launch of its own in front of the diffusion, which it then calls
// without the zeroing: a change of the order here is a change there.)
int step(sfl_context *c, float dt, float dx, int iters, float omega)
{
    SFL_TRY(sfl_advect_velocity(c, dt, 1));                                              // item 1
    SFL_TRY(apply_queued_forces(c));                                                     // item 2
    SFL_TRY(diffuse(c, c->viscosity.nu, dt, dx, c->viscosity.sweeps, true));             // items 3 and 3a
    SFL_TRY(sfl_calculate_divergence(c, dx));                                            // item 4
    SFL_TRY(sfl_poisson_solve(c, dx, iters, omega));                                     // item 5
    SFL_TRY(sfl_subtract_gradient(c, dx));                                               // item 6
    SFL_TRY(sfl_advect_color(c, dt, 0));                                                 // item 7
    return SFL_OK;
}

}  // namespace

extern "C" {

int sfl_set_viscosity(sfl_context *c, float nu, int sweeps)
{
    const char *call = "sfl_set_viscosity";
    SFL_TRY(check_numbers(call, nu, sweeps));   // (what needs no context comes first: it answers on a box without a GPU too)
    if (!c) return fail(SFL_ERR_INVALID, "%s: ctx is NULL", call);
    ContextViscosity &v = c->viscosity;
    if (nu == 0.0f || sweeps == 0) {   // clear: the calls launch what they launched before (the third buffer stays with the context)
        v.set = false;
        v.nu = 0.0f;
        v.sweeps = 0;
        v.step = nullptr;
        return SFL_OK;
    }
    SFL_TRY(check_whole_domain(c, call, "nothing set"));
    if (c->openings.set)
        return fail(SFL_ERR_STATE, "%s: the context has openings set (sfl_set_openings) and the viscous kernels do not know them: nothing set; "
                    "clear the openings first (sfl_set_openings(ctx, NULL, 0, 0))", call);
    v.set = true;
    v.nu = nu;
    v.sweeps = sweeps;
    v.step = step;
    return SFL_OK;
}

int sfl_viscosity_info(sfl_context *c, float *nu, int *sweeps)
{
    if (!c) return fail(SFL_ERR_INVALID, "sfl_viscosity_info: ctx is NULL");
    if (nu) *nu = c->viscosity.set ? c->viscosity.nu : 0.0f;
    if (sweeps) *sweeps = c->viscosity.set ? c->viscosity.sweeps : 0;
    return SFL_OK;
}

int sfl_diffuse_velocity(sfl_context *c, float nu, float dt, float dx, int sweeps)
{
    const char *call = "sfl_diffuse_velocity";
    SFL_TRY(check_numbers(call, nu, sweeps));
    if (!c) return fail(SFL_ERR_INVALID, "%s: ctx is NULL", call);
    if (nu > 0.0f) SFL_TRY(check_whole_domain(c, call, "nothing launched"));
    SFL_TRY(settle_color(c, true));
    SFL_TRY(check_wait_error(c));
    return diffuse(c, nu, dt, dx, sweeps, false);
}

}  // extern "C"
