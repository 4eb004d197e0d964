// openings.cpp -- inflow and outflow cells on the rim of the members of a batch (include/sfl.h "OPENINGS";
// sfl_batch_set_openings, _set_inflow, _openings_info, _openings_download, _inflow_download): the user's map checked and,
// with the mask of the solids where one is set, turned into one open code per cell on the host (open_codes below), kept on
// the device beside the members' inflow velocities, and the launches of batch_openings.hip that the step, solve and
// statistics calls of batch.cpp make while a map is set.  Host C++ only.
//
// As with the solids, batch.cpp does not call into this unit: what a batch holds of its openings is plain data on the struct
// (batch_state.h Openings; freed by the destroy path), and the launches are reached through its pointers, set here while a
// map is set and null otherwise -- then a call launches exactly what it launched before there were openings.  The code bytes
// of the solids are read here and never written: the kernels that read them are handed what they were handed before.
#include "batch_state.h"

#include <cmath>

using sfl::host::fail;

namespace sfl {
namespace host {

std::vector<uint8_t> solid_codes(const uint8_t *mask, int dim_x, int dim_y, size_t members);   // (solids.cpp)

// The side of the domain that rim cell (i, j) looks out of, as the bit of that neighbour (1 W, 2 E, 4 S, 8 N); 0 for an
// interior cell and for a corner, which may carry no opening.
int open_side(int i, int j, int dim_x, int dim_y)
{
    const int w = i == 0, e = i == dim_x - 1, s = j == 0, n = j == dim_y - 1;
    if (w + e + s + n != 1) return 0;
    return w | e << 1 | s << 2 | n << 3;
}

// The first cell of `members` maps that may not hold what it holds: a byte above 2, or a nonzero byte on a corner or an
// interior cell.  Returns false and fills the message, or true.
bool check_open_map(const uint8_t *open, int dim_x, int dim_y, size_t members, char *why, size_t why_bytes)
{
    const size_t cells = (size_t)dim_x * (size_t)dim_y;
    for (size_t m = 0; m < members; ++m)
        for (int j = 0; j < dim_y; ++j)
            for (int i = 0; i < dim_x; ++i) {
                const int v = open[m * cells + (size_t)j * dim_x + i];
                if (!v) continue;
                const bool rim = i == 0 || j == 0 || i == dim_x - 1 || j == dim_y - 1;
                const char *what = v > SFL_OPEN_OUTFLOW ? "is neither 0, SFL_OPEN_INFLOW (1) nor SFL_OPEN_OUTFLOW (2)"
                                   : !rim               ? "is an interior cell: an opening lies on the rim of the grid"
                                   : !open_side(i, j, dim_x, dim_y) ? "is a corner: it has two neighbours outside the domain, an opening has one"
                                                                    : nullptr;
                if (!what) continue;
                snprintf(why, why_bytes, "map %zu, cell (%d, %d) holds %d and %s", m, i, j, v, what);
                return false;
            }
    return true;
}

// The open codes of `members` members: the code byte of the solids below (codes: member stride code_stride, 0 = shared),
// and above it, in a FLUID cell whose map byte (open: member stride open_stride) is nonzero, the open side in bits 8..11
// and bit 12 for an outflow.  Counts the live cells of both kinds.
std::vector<uint16_t> open_codes(const uint8_t *codes, size_t code_stride, const uint8_t *open, size_t open_stride, int dim_x, int dim_y,
                                 size_t members, int64_t *inflow_cells, int64_t *outflow_cells)
{
    const size_t cells = (size_t)dim_x * (size_t)dim_y;
    std::vector<uint16_t> out(members * cells);
    int64_t in = 0, off = 0;
    for (size_t m = 0; m < members; ++m)
        for (int j = 0; j < dim_y; ++j)
            for (int i = 0; i < dim_x; ++i) {
                const size_t c = (size_t)j * dim_x + i;
                const int code = codes[m * code_stride + c], v = open[m * open_stride + c];
                int high = 0;
                if (v && (code & 16)) {
                    high = open_side(i, j, dim_x, dim_y) << 8 | (v == SFL_OPEN_OUTFLOW ? 1 << 12 : 0);
                    ++(v == SFL_OPEN_OUTFLOW ? off : in);
                }
                out[m * cells + c] = (uint16_t)(code | high);
            }
    *inflow_cells = in;
    *outflow_cells = off;
    return out;
}

}  // namespace host
}  // namespace sfl

namespace {

sfl::BatchOpenings openings_of(const sfl_batch *b)
{
    return sfl::BatchOpenings{b->openings.d_codes, b->openings.codes_per_member ? b->cells : 0, b->openings.d_inflow};
}

int step(sfl_batch *b, bool each, const sfl::BatchStep &a)
{
    if (b->openings.profile_step) return b->openings.profile_step(b, each, a);   // (an inflow profile is held: inflow.cpp)
    if (each)
        HIP_TRY(sfl::launch_batch_open_step_each(b->stream, a, openings_of(b), b->batch, b->d_members, b->d_report));
    else
        HIP_TRY(sfl::launch_batch_open_step(b->stream, a, openings_of(b), b->batch));
    return SFL_OK;
}

int solve(sfl_batch *b, bool each, int iters, sfl::SorParams prm)
{
    if (each)
        HIP_TRY(sfl::launch_batch_open_solve_each(b->stream, b->p, b->div, openings_of(b), b->dim_x, b->dim_y, b->batch, b->d_members, b->d_report));
    else
        HIP_TRY(sfl::launch_batch_open_solve(b->stream, b->p, b->div, openings_of(b), b->dim_x, b->dim_y, b->batch, iters, prm));
    return SFL_OK;
}

int stats(sfl_batch *b, float two_dx_inv, const float *d_member_two_dx_inv)
{
    HIP_TRY(sfl::launch_open_velocity_stats(b->stream, b->d_stats, b->vel, openings_of(b), b->dim_x, b->dim_y, b->batch, two_dx_inv,
                                            d_member_two_dx_inv));
    return SFL_OK;
}

int restage(sfl_batch *b);

void set_hooks(sfl_batch *b, bool on)
{
    sfl_batch::Openings &o = b->openings;
    o.set = on;
    o.step = on ? step : nullptr;
    o.solve = on ? solve : nullptr;
    o.stats = on ? stats : nullptr;
    o.restage = on ? restage : nullptr;
}

// everything gone: the batch launches what it launched before (launches in flight may still read the codes)
int clear(sfl_batch *b)
{
    sfl_batch::Openings &o = b->openings;
    if (o.d_codes || o.d_inflow) HIP_TRY(hipStreamSynchronize(b->stream));
    if (o.d_codes) (void)hipFree(o.d_codes);
    if (o.d_inflow) (void)hipFree(o.d_inflow);
    if (o.d_profile) (void)hipFree(o.d_profile);
    if (o.d_flux) (void)hipFree(o.d_flux);
    o = sfl_batch::Openings{};
    return SFL_OK;
}

// a new map: the inflow profile goes ("INFLOW PROFILES AND FLUX"; the stream is idle)
void drop_profile(sfl_batch *b)
{
    sfl_batch::Openings &o = b->openings;
    if (o.d_profile) (void)hipFree(o.d_profile);
    o.d_profile = nullptr;
    o.d_profile_bytes = 0;
    o.profile_table = sfl::BatchProfile{nullptr, nullptr, nullptr};
    o.profile.clear();
    o.profile_on = o.profile_shared = false;
    o.profile_step = nullptr;
    o.profile_restage = nullptr;
}

// a device allocation of the call `call`; nothing is held on failure
int device_alloc(void **mem, size_t bytes, const char *call, const char *what)
{
    const hipError_t e = hipMalloc(mem, bytes);
    if (e == hipSuccess) return SFL_OK;
    (void)hipGetLastError();   // (so that the next launch's check does not report this failure again)
    *mem = nullptr;
    return fail(e == hipErrorOutOfMemory ? SFL_ERR_NOMEM : SFL_ERR_HIP, "%s: hipMalloc of %zu bytes of %s failed: %s", call, bytes, what,
                hipGetErrorString(e));
}

// The open codes formed from the map held and the solids as they stand, and copied to the device.  While it runs the
// openings are off: a failure leaves the batch without them rather than with stale codes.
int stage_codes(sfl_batch *b, const char *call)
{
    sfl_batch::Openings &o = b->openings;
    const bool solids = b->solids.set, solids_each = solids && b->solids.per_member;
    const size_t cells = b->cells, members = (o.per_member || solids_each) ? (size_t)b->batch : 1;
    set_hooks(b, false);
    HIP_TRY(hipStreamSynchronize(b->stream));   // launches in flight may still read the codes this call replaces
    std::vector<uint8_t> bytes;
    if (solids) {   // the code bytes as the solids' kernels read them
        bytes.resize(solids_each ? (size_t)b->batch * cells : cells);
        HIP_TRY(hipMemcpyAsync(bytes.data(), b->solids.d_codes, bytes.size(), hipMemcpyDeviceToHost, b->stream));
        HIP_TRY(hipStreamSynchronize(b->stream));
    } else {   // an all-fluid grid
        const std::vector<uint8_t> none(cells, 0);
        bytes = sfl::host::solid_codes(none.data(), b->dim_x, b->dim_y, 1);
    }
    const std::vector<uint16_t> codes = sfl::host::open_codes(bytes.data(), solids_each ? cells : 0, o.map.data(), o.per_member ? cells : 0, b->dim_x,
                                                              b->dim_y, members, &o.inflow_cells, &o.outflow_cells);
    if (members == 1) {   // (the counts are over all members)
        o.inflow_cells *= b->batch;
        o.outflow_cells *= b->batch;
    }
    const size_t want = codes.size() * sizeof(uint16_t);
    if (want > o.d_bytes) {
        if (o.d_codes) (void)hipFree(o.d_codes);
        o.d_codes = nullptr;
        o.d_bytes = 0;
        void *mem = nullptr;
        SFL_TRY(device_alloc(&mem, want, call, "open codes"));
        o.d_codes = static_cast<uint16_t *>(mem);
        o.d_bytes = want;
    }
    HIP_TRY(hipMemcpyAsync(o.d_codes, codes.data(), want, hipMemcpyHostToDevice, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));   // (`codes` goes with this call)
    o.codes_per_member = members != 1;
    if (o.profile_restage) SFL_TRY(o.profile_restage(b, codes.data(), members != 1 ? cells : 0));   // (the profile's table names fluid cells only)
    set_hooks(b, true);
    return SFL_OK;
}

// the inflow held, one (x, y) per member, copied to the device behind the launches queued so far
int stage_inflow(sfl_batch *b, const char *call)
{
    sfl_batch::Openings &o = b->openings;
    const size_t bytes = sizeof(float) * 2 * (size_t)b->batch;
    if (!o.d_inflow) {
        void *mem = nullptr;
        SFL_TRY(device_alloc(&mem, bytes, call, "inflow velocities"));
        o.d_inflow = static_cast<float *>(mem);
    }
    HIP_TRY(hipMemcpyAsync(o.d_inflow, o.inflow.data(), bytes, hipMemcpyHostToDevice, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));   // (a later call may rewrite o.inflow)
    return SFL_OK;
}

int restage(sfl_batch *b) { return stage_codes(b, "sfl_batch_set_solids"); }

// inflow: n velocities (x, y), all finite
int check_inflow(int n, const float *inflow, const char *call)
{
    for (int m = 0; m < n; ++m)
        if (!std::isfinite(inflow[2 * m]) || !std::isfinite(inflow[2 * m + 1]))
            return fail(SFL_ERR_INVALID, "%s: the inflow velocity must be finite (member %d: (%g, %g))", call, m, (double)inflow[2 * m],
                        (double)inflow[2 * m + 1]);
    return SFL_OK;
}

void keep_inflow(sfl_batch *b, const float *inflow, int per_member)
{
    sfl_batch::Openings &o = b->openings;
    o.inflow.resize(2 * (size_t)b->batch);
    for (int m = 0; m < b->batch; ++m) {
        o.inflow[2 * m] = inflow[per_member ? 2 * m : 0];
        o.inflow[2 * m + 1] = inflow[per_member ? 2 * m + 1 : 1];
    }
    o.inflow_per_member = per_member != 0;
}

int check_range(const sfl_batch *b, int first, int count, const char *call)
{
    if (first < 0 || count < 0 || (int64_t)first + count > b->batch)
        return fail(SFL_ERR_INVALID, "%s: members [%d, %d + %d) are not inside the batch's [0, %d)", call, first, first, count, b->batch);
    return SFL_OK;
}

}  // namespace

extern "C" {

int sfl_batch_set_openings(sfl_batch *b, const uint8_t *open, int per_member, const float *inflow, int inflow_per_member)
{
    const char *call = "sfl_batch_set_openings";
    if (per_member != 0 && per_member != 1) return fail(SFL_ERR_INVALID, "%s: per_member must be 0 or 1 (got %d)", call, per_member);
    if (inflow_per_member != 0 && inflow_per_member != 1)
        return fail(SFL_ERR_INVALID, "%s: inflow_per_member must be 0 or 1 (got %d)", call, inflow_per_member);
    // (what needs no batch comes first: it answers on a box without a GPU too -- a shared inflow is one (x, y))
    if (open && inflow && !inflow_per_member) SFL_TRY(check_inflow(1, inflow, call));
    if (!b) return fail(SFL_ERR_INVALID, "%s: batch is NULL", call);
    if (open) {
        if (!inflow) return fail(SFL_ERR_INVALID, "%s: inflow is NULL (a map needs an inflow velocity, (0, 0) included)", call);
        char why[200];
        if (!sfl::host::check_open_map(open, b->dim_x, b->dim_y, per_member ? (size_t)b->batch : 1, why, sizeof why))
            return fail(SFL_ERR_INVALID, "%s: %s", call, why);
        SFL_TRY(check_inflow(inflow_per_member ? b->batch : 1, inflow, call));
        if (b->large)
            return fail(SFL_ERR_STATE, "%s: a batch of sfl_batch_create_large has no openings: its kernels do not know them (members of at most "
                        "%d cells, made by sfl_batch_create, do)", call, sfl::kSmallGridMaxCells);
        if (b->history.on)
            return fail(SFL_ERR_STATE, "%s: a history is on and its samples do not know openings: nothing set; stop it first "
                        "(sfl_batch_history_stop)", call);
        if (b->rec.on && b->rec.view_on && b->rec.view.what == SFL_VIEW_DIVERGENCE)
            return fail(SFL_ERR_STATE, "%s: the recorder draws the divergence view, which does not know openings: nothing set; record "
                        "another view or the dye first (sfl_batch_record_view)", call);
        if (b->viscosity.set)
            return fail(SFL_ERR_STATE, "%s: viscosity is set (sfl_batch_set_viscosity) and the viscous kernels do not know openings: nothing set; "
                        "clear it first (sfl_batch_set_viscosity(b, NULL, 0, 0))", call);
    }
    HIP_TRY(hipSetDevice(b->device));
    if (!open) return clear(b);
    sfl_batch::Openings &o = b->openings;
    if (o.profile_on) {   // (launches in flight may still read its table)
        HIP_TRY(hipStreamSynchronize(b->stream));
        drop_profile(b);
    }
    o.map.assign(open, open + (per_member ? (size_t)b->batch : 1) * b->cells);
    o.per_member = per_member != 0;
    keep_inflow(b, inflow, inflow_per_member);
    set_hooks(b, false);
    SFL_TRY(stage_inflow(b, call));
    return stage_codes(b, call);
}

int sfl_batch_set_inflow(sfl_batch *b, const float *inflow, int per_member)
{
    const char *call = "sfl_batch_set_inflow";
    if (per_member != 0 && per_member != 1) return fail(SFL_ERR_INVALID, "%s: per_member must be 0 or 1 (got %d)", call, per_member);
    if (inflow && !per_member) SFL_TRY(check_inflow(1, inflow, call));   // (needs no batch)
    if (!b) return fail(SFL_ERR_INVALID, "%s: batch is NULL", call);
    if (!inflow) return fail(SFL_ERR_INVALID, "%s: inflow is NULL", call);
    SFL_TRY(check_inflow(per_member ? b->batch : 1, inflow, call));
    if (!b->openings.set)
        return fail(SFL_ERR_STATE, "%s: the batch has no openings set: nothing changed; set a map with its inflow first (sfl_batch_set_openings)", call);
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(b->stream));   // launches in flight may still read the velocities this call replaces
    keep_inflow(b, inflow, per_member);
    return stage_inflow(b, call);
}

int sfl_batch_openings_info(sfl_batch *b, int *set, int *per_member, int *inflow_per_member, int64_t *inflow_cells, int64_t *outflow_cells)
{
    if (!b) return fail(SFL_ERR_INVALID, "sfl_batch_openings_info: batch is NULL");
    const sfl_batch::Openings &o = b->openings;
    if (set) *set = o.set ? 1 : 0;
    if (per_member) *per_member = o.set && o.per_member ? 1 : 0;
    if (inflow_per_member) *inflow_per_member = o.set && o.inflow_per_member ? 1 : 0;
    if (inflow_cells) *inflow_cells = o.set ? o.inflow_cells : 0;
    if (outflow_cells) *outflow_cells = o.set ? o.outflow_cells : 0;
    return SFL_OK;
}

int sfl_batch_openings_download(sfl_batch *b, int first, int count, uint8_t *host, size_t bytes)
{
    const char *call = "sfl_batch_openings_download";
    if (!b) return fail(SFL_ERR_INVALID, "%s: batch is NULL", call);
    SFL_TRY(check_range(b, first, count, call));
    const size_t want = (size_t)count * b->cells;
    if (bytes != want) return fail(SFL_ERR_INVALID, "%s: the maps of %d members are %zu bytes, got %zu", call, count, want, bytes);
    if (count == 0) return SFL_OK;
    if (!host) return fail(SFL_ERR_INVALID, "%s: host is NULL", call);
    const sfl_batch::Openings &o = b->openings;
    for (int m = 0; m < count; ++m) {
        if (!o.set)
            memset(host + (size_t)m * b->cells, 0, b->cells);
        else
            memcpy(host + (size_t)m * b->cells, o.map.data() + (o.per_member ? (size_t)(first + m) * b->cells : 0), b->cells);
    }
    return SFL_OK;
}

int sfl_batch_inflow_download(sfl_batch *b, int first, int count, float *host, size_t bytes)
{
    const char *call = "sfl_batch_inflow_download";
    if (!b) return fail(SFL_ERR_INVALID, "%s: batch is NULL", call);
    SFL_TRY(check_range(b, first, count, call));
    const size_t want = (size_t)count * 2 * sizeof(float);
    if (bytes != want) return fail(SFL_ERR_INVALID, "%s: the inflow velocities of %d members are %zu bytes, got %zu", call, count, want, bytes);
    if (count == 0) return SFL_OK;
    if (!host) return fail(SFL_ERR_INVALID, "%s: host is NULL", call);
    if (!b->openings.set)
        memset(host, 0, bytes);
    else
        memcpy(host, b->openings.inflow.data() + 2 * (size_t)first, bytes);
    return SFL_OK;
}

}  // extern "C"
