// viscous.cpp -- viscosity of a batch (include/sfl.h "VISCOSITY"; sfl_batch_set_viscosity, _viscosity_info,
// _viscosity_download): every member's nu kept on the host, turned into one record per member (a, c, sweeps) for the
// dt and dx of each step call, and the launches of batch_viscous.hip that the step calls of batch.cpp make while a
// viscosity is set.  Host C++ only.
//
// The calls of batch.cpp live in a unit that the host test harnesses link without this one, so they do not call into it:
// what a batch holds of its viscosity is plain data on the struct (batch_state.h Viscosity; freed by the destroy path), and
// the staging and the launches are reached through its two pointers, set here while a viscosity is set and null
// otherwise -- then a call launches exactly what it launched before there was viscosity.
#include "batch_state.h"
#include "diffuse_tile.h"
#include "viscous_kernels.h"

#include <cmath>

using sfl::host::fail;

namespace {

sfl::BatchSolids solids_of(const sfl_batch *b)
{
    return sfl::BatchSolids{b->solids.d_codes, b->solids.per_member ? b->cells : 0};
}

// The members' records for one step call, copied to the device behind the launches queued so far: a and c by the
// header's expressions from member m's nu and the call's dt and dx (params: member m's own).  nu == 0 stores sweeps 0:
// the member skips the item.  The device table has its final size from the first call on and is written in stream order;
// a pinned slot is rewritten only after its last copy has completed (the rule of batch.cpp stage_members).
int stage(sfl_batch *b, float dt, float dx, const sfl_member_params *params)
{
    sfl_batch::Viscosity &v = b->viscosity;
    const size_t bytes = sizeof(sfl::BatchViscous) * (size_t)b->batch;
    sfl_batch::Stage &st = v.stage_slot[v.slot];
    v.slot ^= 1;
    if (!st.copied) HIP_TRY(hipEventCreateWithFlags(&st.copied, hipEventDisableTiming));
    if (st.pending) {
        HIP_TRY(hipEventSynchronize(st.copied));
        st.pending = false;
    }
    if (!st.host) {
        HIP_TRY(hipHostMalloc(&st.host, bytes, hipHostMallocDefault));
        st.bytes = bytes;
    }
    if (!v.d_table) HIP_TRY(hipMalloc(&v.d_table, bytes));
    sfl::BatchViscous *rec = static_cast<sfl::BatchViscous *>(st.host);
    for (int m = 0; m < b->batch; ++m) {
        const sfl::diffuse::Coefficients k = sfl::diffuse::coefficients(v.nu[m], params ? params[m].dt : dt, params ? params[m].dx : dx);
        rec[m].a = k.a;
        rec[m].c = k.c;
        rec[m].sweeps = v.nu[m] == 0.0f ? 0 : v.sweeps;
    }
    HIP_TRY(hipMemcpyAsync(v.d_table, st.host, bytes, hipMemcpyHostToDevice, b->stream));
    HIP_TRY(hipEventRecord(st.copied, b->stream));
    st.pending = true;
    return SFL_OK;
}

// one step is due: launch it (each: by the records of d_members, and the update norm into d_report), by the solids' rule
// where a mask is set
int step(sfl_batch *b, bool each, const sfl::BatchStep &a)
{
    const sfl::BatchViscous *table = static_cast<const sfl::BatchViscous *>(b->viscosity.d_table);
    if (b->solids.set) {
        if (each)
            HIP_TRY(sfl::launch_batch_viscous_solid_step_each(b->stream, a, solids_of(b), table, b->batch, b->d_members, b->d_report));
        else
            HIP_TRY(sfl::launch_batch_viscous_solid_step(b->stream, a, solids_of(b), table, b->batch));
    } else if (each)
        HIP_TRY(sfl::launch_batch_viscous_step_each(b->stream, a, table, b->batch, b->d_members, b->d_report));
    else
        HIP_TRY(sfl::launch_batch_viscous_step(b->stream, a, table, b->batch));
    return SFL_OK;
}

}  // namespace

extern "C" {

int sfl_batch_set_viscosity(sfl_batch *b, const float *nu, int per_member, int sweeps)
{
    const char *call = "sfl_batch_set_viscosity";
    // (what needs no batch comes first: it answers on a box without a GPU too -- a shared nu is one float)
    if (per_member != 0 && per_member != 1) return fail(SFL_ERR_INVALID, "%s: per_member must be 0 or 1 (got %d)", call, per_member);
    if (sweeps < 0) return fail(SFL_ERR_INVALID, "%s: sweeps must be >= 0 (got %d)", call, sweeps);
    if (nu && !per_member && (std::isnan(nu[0]) || nu[0] < 0.0f))
        return fail(SFL_ERR_INVALID, "%s: nu must be >= 0 and not a NaN (got %g): nothing set", call, (double)nu[0]);
    if (!b) return fail(SFL_ERR_INVALID, "%s: batch is NULL", call);
    for (int m = 0; nu && per_member && m < b->batch; ++m)
        if (std::isnan(nu[m]) || nu[m] < 0.0f)
            return fail(SFL_ERR_INVALID, "%s: member %d: nu must be >= 0 and not a NaN (got %g): nothing set", call, m, (double)nu[m]);
    sfl_batch::Viscosity &v = b->viscosity;
    if (!nu) {   // clear: the calls launch what they launched before (the table and the slots stay with the batch)
        v.set = v.per_member = false;
        v.sweeps = 0;
        v.nu.clear();
        v.stage = nullptr;
        v.step = nullptr;
        return SFL_OK;
    }
    if (b->large)
        return fail(SFL_ERR_STATE, "%s: a batch of sfl_batch_create_large has no viscosity: its 8 B of LDS per cell leave no room for u0 (members of "
                    "at most %d cells, made by sfl_batch_create, have it)", call, sfl::kSmallGridMaxCells);
    if (b->openings.set)
        return fail(SFL_ERR_STATE, "%s: the batch has openings set (sfl_batch_set_openings) and the viscous kernels do not know them: nothing set; "
                    "clear the openings first (sfl_batch_set_openings(b, NULL, 0, NULL, 0))", call);
    v.nu.assign((size_t)b->batch, nu[0]);
    if (per_member) v.nu.assign(nu, nu + b->batch);
    v.set = true;
    v.per_member = per_member != 0;
    v.sweeps = sweeps;
    v.stage = stage;
    v.step = step;
    return SFL_OK;
}

int sfl_batch_viscosity_info(sfl_batch *b, int *set, int *per_member, int *sweeps)
{
    if (!b) return fail(SFL_ERR_INVALID, "sfl_batch_viscosity_info: batch is NULL");
    if (set) *set = b->viscosity.set ? 1 : 0;
    if (per_member) *per_member = b->viscosity.set && b->viscosity.per_member ? 1 : 0;
    if (sweeps) *sweeps = b->viscosity.set ? b->viscosity.sweeps : 0;
    return SFL_OK;
}

int sfl_batch_viscosity_download(sfl_batch *b, int first, int count, float *host, size_t bytes)
{
    const char *call = "sfl_batch_viscosity_download";
    if (!b) return fail(SFL_ERR_INVALID, "%s: batch is NULL", call);
    if (first < 0 || count < 0 || (int64_t)first + count > b->batch)
        return fail(SFL_ERR_INVALID, "%s: members [%d, %d + %d) are not inside the batch's [0, %d)", call, first, first, count, b->batch);
    const size_t want = (size_t)count * sizeof(float);
    if (bytes != want) return fail(SFL_ERR_INVALID, "%s: nu of %d members is %zu bytes, got %zu", call, count, want, bytes);
    if (count == 0) return SFL_OK;
    if (!host) return fail(SFL_ERR_INVALID, "%s: host is NULL", call);
    for (int k = 0; k < count; ++k) host[k] = b->viscosity.set ? b->viscosity.nu[(size_t)first + k] : 0.0f;
    return SFL_OK;
}

}  // extern "C"
