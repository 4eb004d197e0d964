// solids.cpp -- solid cells inside the members of a batch (include/sfl.h "SOLIDS"; sfl_batch_set_solids, _solids_info,
// _solids_download): the user's mask turned into one code byte per cell on the host (solid_codes below), kept on the
// device, and the launches of batch_solids.hip that the step, solve and statistics calls of batch.cpp make while a mask is
// set.  Host C++ only.
//
// The calls of batch.cpp live in a unit that the host test harnesses link without this one, so they do not call into it:
// what a batch holds of its solids is plain data on the struct (batch_state.h Solids; freed by the destroy path), and the
// launches are reached through its three pointers, set here while a mask is set and null otherwise -- then a call launches
// exactly what it launched before there were solids.
#include "batch_state.h"

using sfl::host::fail;

namespace sfl {
namespace host {

// The code bytes of `members` masks of dim_y x dim_x bytes (nonzero = solid), member-major, cell (i, j) at dim_x * j + i:
// bit 0 W, 1 E, 2 S, 3 N neighbour present -- inside the domain and fluid --, bit 4 the cell is fluid; a solid cell's byte is 0.
std::vector<uint8_t> solid_codes(const uint8_t *mask, int dim_x, int dim_y, size_t members)
{
    const size_t cells = (size_t)dim_x * (size_t)dim_y;
    std::vector<uint8_t> codes(members * cells);
    for (size_t m = 0; m < members; ++m) {
        const uint8_t *s = mask + m * cells;
        uint8_t *out = codes.data() + m * cells;
        for (int j = 0; j < dim_y; ++j)
            for (int i = 0; i < dim_x; ++i) {
                const size_t c = (size_t)j * dim_x + i;
                if (s[c]) {
                    out[c] = 0;
                    continue;
                }
                const int w = i > 0 && !s[c - 1], e = i < dim_x - 1 && !s[c + 1];
                const int so = j > 0 && !s[c - dim_x], n = j < dim_y - 1 && !s[c + dim_x];
                out[c] = (uint8_t)(w | e << 1 | so << 2 | n << 3 | 16);
            }
    }
    return codes;
}

}  // namespace host
}  // namespace sfl

namespace {

sfl::BatchSolids solids_of(const sfl_batch *b)
{
    return sfl::BatchSolids{b->solids.d_codes, b->solids.per_member ? b->cells : 0};
}

int step(sfl_batch *b, bool each, const sfl::BatchStep &a)
{
    if (each)
        HIP_TRY(sfl::launch_batch_solid_step_each(b->stream, a, solids_of(b), b->batch, b->d_members, b->d_report));
    else
        HIP_TRY(sfl::launch_batch_solid_step(b->stream, a, solids_of(b), b->batch));
    return SFL_OK;
}

int solve(sfl_batch *b, bool each, int iters, sfl::SorParams prm)
{
    if (each)
        HIP_TRY(sfl::launch_batch_solid_solve_each(b->stream, b->p, b->div, solids_of(b), b->dim_x, b->dim_y, b->batch, b->d_members, b->d_report));
    else
        HIP_TRY(sfl::launch_batch_solid_solve(b->stream, b->p, b->div, solids_of(b), b->dim_x, b->dim_y, b->batch, iters, prm));
    return SFL_OK;
}

int stats(sfl_batch *b, float two_dx_inv, const float *d_member_two_dx_inv)
{
    HIP_TRY(sfl::launch_solid_velocity_stats(b->stream, b->d_stats, b->vel, solids_of(b), b->dim_x, b->dim_y, b->batch, two_dx_inv,
                                             d_member_two_dx_inv));
    return SFL_OK;
}

void set_hooks(sfl_batch *b)
{
    const bool on = b->solids.set;
    b->solids.step = on ? step : nullptr;
    b->solids.solve = on ? solve : nullptr;
    b->solids.stats = on ? stats : nullptr;
}

}  // namespace

extern "C" {

int sfl_batch_set_solids(sfl_batch *b, const uint8_t *mask, int per_member)
{
    const char *call = "sfl_batch_set_solids";
    if (per_member != 0 && per_member != 1) return fail(SFL_ERR_INVALID, "%s: per_member must be 0 or 1 (got %d)", call, per_member);
    if (!b) return fail(SFL_ERR_INVALID, "%s: batch is NULL", call);
    if (b->large)
        return fail(SFL_ERR_STATE, "%s: a batch of sfl_batch_create_large has no solid cells: its kernels do not know them (members of at most "
                    "%d cells, made by sfl_batch_create, do)", call, sfl::kSmallGridMaxCells);
    if (mask && b->history.on)
        return fail(SFL_ERR_STATE, "%s: a history is on and its samples do not know solid cells: nothing set; stop it first "
                    "(sfl_batch_history_stop)", call);
    if (mask && b->rec.on && b->rec.view_on && b->rec.view.what == SFL_VIEW_DIVERGENCE)
        return fail(SFL_ERR_STATE, "%s: the recorder draws the divergence view, which does not know solid cells: nothing set; record "
                    "another view or the dye first (sfl_batch_record_view)", call);
    HIP_TRY(hipSetDevice(b->device));
    sfl_batch::Solids &s = b->solids;
    if (!mask) {   // clear: the calls launch what they launched before; launches in flight may still read the bytes
        if (s.d_codes) {
            HIP_TRY(hipStreamSynchronize(b->stream));
            (void)hipFree(s.d_codes);
        }
        s = sfl_batch::Solids{};
        if (b->walls.drop) b->walls.drop(b);   // (a wall is a solid cell: the table goes with the mask)
        if (b->openings.restage) SFL_TRY(b->openings.restage(b));   // (the openings' codes: every cell is fluid again)
        return SFL_OK;
    }
    const size_t members = per_member ? (size_t)b->batch : 1, bytes = members * b->cells;
    const std::vector<uint8_t> codes = sfl::host::solid_codes(mask, b->dim_x, b->dim_y, members);
    HIP_TRY(hipStreamSynchronize(b->stream));   // launches in flight may still read the bytes this call replaces
    if (bytes > s.d_bytes) {
        if (s.d_codes) (void)hipFree(s.d_codes);
        s = sfl_batch::Solids{};   // no solids unless the bytes are there
        void *mem = nullptr;
        const hipError_t e = hipMalloc(&mem, bytes);
        if (e != hipSuccess) {
            (void)hipGetLastError();   // (so that the next launch's check does not report this failure again)
            return fail(e == hipErrorOutOfMemory ? SFL_ERR_NOMEM : SFL_ERR_HIP, "%s: hipMalloc of %zu code bytes failed: %s", call, bytes,
                        hipGetErrorString(e));
        }
        s.d_codes = static_cast<uint8_t *>(mem);
        s.d_bytes = bytes;
    }
    s.set = false;
    set_hooks(b);
    HIP_TRY(hipMemcpyAsync(s.d_codes, codes.data(), bytes, hipMemcpyHostToDevice, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));   // (`codes` goes with this call)
    s.set = true;
    s.per_member = per_member != 0;
    set_hooks(b);
    if (b->walls.drop) b->walls.drop(b);   // (the table was checked against the mask this call replaced: it goes)
    if (b->openings.restage) SFL_TRY(b->openings.restage(b));   // (an opening counts only where the cell is fluid)
    return SFL_OK;
}

int sfl_batch_solids_info(sfl_batch *b, int *set, int *per_member)
{
    if (!b) return fail(SFL_ERR_INVALID, "sfl_batch_solids_info: batch is NULL");
    if (set) *set = b->solids.set ? 1 : 0;
    if (per_member) *per_member = b->solids.set && b->solids.per_member ? 1 : 0;
    return SFL_OK;
}

int sfl_batch_solids_download(sfl_batch *b, int first, int count, uint8_t *host, size_t bytes)
{
    const char *call = "sfl_batch_solids_download";
    if (!b) return fail(SFL_ERR_INVALID, "%s: batch is NULL", call);
    if (first < 0 || count < 0 || (int64_t)first + count > b->batch)
        return fail(SFL_ERR_INVALID, "%s: members [%d, %d + %d) are not inside the batch's [0, %d)", call, first, first, count, b->batch);
    const size_t want = (size_t)count * b->cells;
    if (bytes != want) return fail(SFL_ERR_INVALID, "%s: the masks of %d members are %zu bytes, got %zu", call, count, want, bytes);
    if (count == 0) return SFL_OK;
    if (!host) return fail(SFL_ERR_INVALID, "%s: host is NULL", call);
    if (!b->solids.set) {   // no solid cell anywhere
        memset(host, 0, bytes);
        return SFL_OK;
    }
    HIP_TRY(hipSetDevice(b->device));
    // the code bytes of the members asked for (a shared mask: one member's, repeated), then solid = not fluid
    const bool each = b->solids.per_member;
    const size_t got = each ? bytes : b->cells;
    HIP_TRY(hipMemcpyAsync(host, b->solids.d_codes + (each ? (size_t)first * b->cells : 0), got, hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    for (size_t c = 0; c < got; ++c) host[c] = (host[c] & 16) ? 0 : 1;
    for (int m = 1; m < count && !each; ++m) memcpy(host + (size_t)m * b->cells, host, b->cells);
    return SFL_OK;
}

}  // extern "C"
