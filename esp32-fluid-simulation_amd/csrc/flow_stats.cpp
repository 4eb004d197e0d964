// flow_stats.cpp -- what the flow a whole-domain context holds looks like: sfl_flow_stats (include/sfl.h).  One streaming
// pass over the velocity, one over the dye (flow_stats.hip), their record copied to the context's pinned one, one wait.
// Host C++ only.  The batches' entry points live with struct sfl_batch (batch.cpp) and launch the same kernels.
#include "context.h"
#include "stats_kernels.h"

using namespace sfl::host;

static_assert(sizeof(struct sfl_flow_stats) == 40 && offsetof(struct sfl_flow_stats, what) == 12 && offsetof(struct sfl_flow_stats, dye_sum) == 16,
              "sfl_flow_stats: 40 bytes, offsets 0, 4, 8, 12, 16");

// the device record and its pinned host copy: allocated at the first call, kept with the context (sfl_destroy frees them)
static int ensure_records(sfl_context *c)
{
    if (!c->d_stats) HIP_TRY(hipMalloc((void **)&c->d_stats, sizeof(struct sfl_flow_stats)));
    if (!c->h_stats) HIP_TRY(hipHostMalloc((void **)&c->h_stats, sizeof(struct sfl_flow_stats), hipHostMallocDefault));
    return SFL_OK;
}

extern "C" {

int sfl_flow_stats(sfl_context *ctx, int what, float dx, struct sfl_flow_stats *out)
{
    if (what == 0 || (what & ~(SFL_STATS_VELOCITY | SFL_STATS_DYE)))   // (first: it needs no context to be wrong)
        return fail(SFL_ERR_INVALID, "what must be SFL_STATS_VELOCITY (1), SFL_STATS_DYE (2) or both (got %d)", what);
    if (!ctx || !out) return fail(SFL_ERR_INVALID, "NULL argument");
    if (ctx->nranks != 1)   // (a slab's figures would need a reduction over the ranks)
        return fail(SFL_ERR_STATE, "sfl_flow_stats: whole-domain contexts only (slab %d/%d)", ctx->rank, ctx->nranks);
    SFL_TRY(settle_color(ctx, true));
    SFL_TRY(check_wait_error(ctx));
    if (what & SFL_STATS_VELOCITY) SFL_TRY(ensure_field(ctx, SFL_FIELD_VELOCITY));
    if (what & SFL_STATS_DYE) SFL_TRY(ensure_field(ctx, SFL_FIELD_COLOR));
    SFL_TRY(use_device(ctx));
    SFL_TRY(ensure_records(ctx));
    const float two_dx_inv = 1.0f / (2.0f * dx);  // finitediff.cpp:36
    sfl::FlowStatsRecord *rec = reinterpret_cast<sfl::FlowStatsRecord *>(ctx->d_stats);
    HIP_TRY(sfl::launch_flow_stats(ctx->stream, rec, what, ctx->vel, ctx->col, ctx->dim_x, ctx->gdim_y, 1, two_dx_inv, nullptr));
    if ((what & SFL_STATS_VELOCITY) && ctx->solids.max_div)   // solid cells set: max_abs_div by item 4 of their rule
        SFL_TRY(ctx->solids.max_div(ctx, two_dx_inv, &rec->max_abs_div));
    HIP_TRY(hipMemcpyAsync(ctx->h_stats, ctx->d_stats, sizeof(struct sfl_flow_stats), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    *out = *ctx->h_stats;
    out->what = (uint32_t)what;
    return SFL_OK;
}

}  // extern "C"
