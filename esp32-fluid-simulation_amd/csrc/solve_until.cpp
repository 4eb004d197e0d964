// solve_until.cpp -- how far a whole-domain context's pressure is from converged, and the solves that go on from it:
// sfl_residual, sfl_poisson_continue, sfl_poisson_solve_until (include/sfl.h).  The update norm is one streaming pass
// (update_norm.hip); a continued solve is run_poisson's warm walk (sor_executor.cpp) or, on a small grid, one launch of its
// own (small_grid.hip); the rule alternates the two and decides on the host.  Host C++ only.
#include "transport.h"
#include "until_kernels.h"

namespace sfl {
namespace host {

// `iters` more iterations on the pressure the context holds
static int continue_poisson(sfl_context *ctx, float dx, int iters, float omega)
{
    if (ctx->solids.solve) return ctx->solids.solve(ctx, dx, iters, omega, true);   // solid cells set: their rule's iterations
    if (!small_grid(ctx)) return run_poisson(ctx, dx, iters, omega, true);
    SFL_TRY(ensure_field(ctx, SFL_FIELD_DIVERGENCE));
    SFL_TRY(ensure_field(ctx, SFL_FIELD_PRESSURE));
    ctx->last_halo = ctx->last_launches = ctx->last_exchanges = 0;
    ctx->last_fuse = 2 * iters;
    ctx->p_ghost_valid = 0;
    if (iters == 0) return SFL_OK;   // the pressure stays as it is
    SFL_TRY(use_device(ctx));
    HIP_TRY(sfl::launch_small_solve_warm(ctx->stream, ctx->p, ctx->div, ctx->dim_x, ctx->gdim_y, iters, sor_params(ctx, dx, omega)));
    ctx->last_launches = 1;
    return SFL_OK;
}

// ---- the update norm and the solve that stops at a tolerance (whole-domain contexts) -------------------------------------
// One pass over p and d (update_norm.hip), its word copied to the context's pinned word, one wait: no allocation per call.
static int read_update_norm(sfl_context *c, float dx, float *norm)
{
    SFL_TRY(ensure_field(c, SFL_FIELD_DIVERGENCE));
    SFL_TRY(ensure_field(c, SFL_FIELD_PRESSURE));
    SFL_TRY(use_device(c));
    if (c->solids.norm)   // solid cells set: the maximum over the fluid cells
        SFL_TRY(c->solids.norm(c, dx, c->d_norm));
    else
        HIP_TRY(sfl::launch_update_norm(c->stream, c->d_norm, c->p, c->div, c->geom, c->g0, c->g1, dx));
    HIP_TRY(hipMemcpyAsync(c->h_norm, c->d_norm, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    memcpy(norm, c->h_norm, sizeof *norm);
    return SFL_OK;
}

// include/sfl.h sfl_poisson_solve_until.  General kernels: p = 0, then a check (a norm read on the host) in front of every
// warm segment of `every` iterations, the last one shortened to the cap; the norm of the pressure the solve ends with is
// always read.  tol < 0 checks nothing: the plain solve and one norm.  Small grids: the rule runs inside ONE launch
// (small_grid.hip), which leaves the norm and the count in the context's device words.
static int run_poisson_until(sfl_context *ctx, float dx, int cap, float omega, float tol, int every, int32_t *iterations, float *norm)
{
    float u = 0.0f;
    int k = 0, launches = 0;
    // (solid cells set: the host loop on every grid, over the masked solve and the masked norm)
    const auto from_zero = [&](int iters) { return ctx->solids.solve ? ctx->solids.solve(ctx, dx, iters, omega, false) : run_poisson(ctx, dx, iters, omega); };
    if (small_grid(ctx) && !ctx->solids.solve) {
        SFL_TRY(ensure_field(ctx, SFL_FIELD_DIVERGENCE));
        SFL_TRY(ensure_field(ctx, SFL_FIELD_PRESSURE));
        SFL_TRY(use_device(ctx));
        ctx->last_halo = ctx->last_exchanges = 0;
        const sfl::SorParams prm = sor_params(ctx, dx, omega);
        HIP_TRY(sfl::launch_small_solve_until(ctx->stream, ctx->p, ctx->div, ctx->dim_x, ctx->gdim_y, cap, prm, tol,
                                              tol < 0.0f ? INT_MAX : every, ctx->d_norm));   // (tol < 0: no check but the last)
        HIP_TRY(hipMemcpyAsync(ctx->h_norm, ctx->d_norm, kNormWords * sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        memcpy(&u, ctx->h_norm, sizeof u);
        k = (int)ctx->h_norm[1];
        launches = 1;
        ctx->last_fuse = 2 * k;
    } else if (tol < 0.0f) {
        SFL_TRY(from_zero(cap));
        launches = ctx->last_launches;
        k = cap;
        SFL_TRY(read_update_norm(ctx, dx, &u));
    } else {
        SFL_TRY(from_zero(0));   // p = 0 (poisson.cpp:117-119): what the check at k = 0 sees
        for (;;) {
            SFL_TRY(read_update_norm(ctx, dx, &u));
            if (k >= cap || !(u > tol)) break;   // !(u > tol): u <= tol, or u is a NaN
            const int segment = std::min(every, cap - k);
            SFL_TRY(continue_poisson(ctx, dx, segment, omega));
            launches += ctx->last_launches;
            k += segment;
        }
    }
    ctx->last_launches = launches;
    ctx->p_ghost_valid = 0;
    if (iterations) *iterations = k;
    if (norm) *norm = u;
    return SFL_OK;
}

}  // namespace host
}  // namespace sfl

using namespace sfl::host;

extern "C" {

// the three calls below: whole-domain contexts (a slab's norm would need a reduction over the ranks, its continued solve a
// halo for the first superstep)
static int whole_domain_only(const sfl_context *c, const char *call)
{
    if (c->nranks != 1)
        return fail(SFL_ERR_STATE, "%s: whole-domain contexts only (slab %d/%d)", call, c->rank, c->nranks);
    return SFL_OK;
}

int sfl_residual(sfl_context *ctx, float dx, float *norm)
{
    if (!ctx || !norm) return fail(SFL_ERR_INVALID, "NULL argument");
    SFL_TRY(whole_domain_only(ctx, "sfl_residual"));
    SFL_TRY(settle_color(ctx, true));
    SFL_TRY(check_wait_error(ctx));
    ctx->p_ghost_valid = 0;
    return read_update_norm(ctx, dx, norm);
}

int sfl_poisson_continue(sfl_context *ctx, float dx, int iters, float omega)
{
    if (!ctx) return fail(SFL_ERR_INVALID, "ctx is NULL");
    if (iters < 0) return fail(SFL_ERR_INVALID, "iters must be >= 0 (got %d)", iters);
    SFL_TRY(whole_domain_only(ctx, "sfl_poisson_continue"));
    SFL_TRY(settle_color(ctx, true));
    SFL_TRY(check_wait_error(ctx));
    ctx->p_ghost_valid = 0;
    return continue_poisson(ctx, dx, iters, omega);
}

int sfl_poisson_solve_until(sfl_context *ctx, float dx, int iters, float omega, float tol, int every, int32_t *iterations,
                            float *norm)
{
    if (!ctx) return fail(SFL_ERR_INVALID, "ctx is NULL");
    if (iters < 0) return fail(SFL_ERR_INVALID, "iters (the cap) must be >= 0 (got %d)", iters);
    if (every < 1) return fail(SFL_ERR_INVALID, "every must be >= 1 (got %d)", every);
    if (tol != tol) return fail(SFL_ERR_INVALID, "tol is a NaN (a negative tol never stops the solve)");
    SFL_TRY(whole_domain_only(ctx, "sfl_poisson_solve_until"));
    SFL_TRY(settle_color(ctx, true));
    SFL_TRY(check_wait_error(ctx));
    return run_poisson_until(ctx, dx, iters, omega, tol, every, iterations, norm);
}

}  // extern "C"
