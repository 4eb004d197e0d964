// context_solids.cpp -- solid cells inside the grid of a whole-domain context (include/sfl.h "SOLIDS OF A CONTEXT";
// sfl_set_solids, _solids_info, _solids_download): the user's mask turned into one code byte per cell on the host
// (solids.cpp solid_codes, members = 1), kept on the device, and the launches of context_solids.hip that the step, the
// operators, the solves, the update norm, the statistics and the history's sample make while a mask is set.  Host C++ only.
//
// Those calls live in units that the host test harnesses link without this one, so they do not call into it: what a
// context holds of its solids is plain data on the struct (context.h ContextSolids; sfl_destroy frees the bytes), and
// the launches are reached through its pointers, set here while a mask is set and null otherwise -- then a call launches
// exactly what it launched before there were solids.
#include "context.h"
#include "solid_kernels.h"
#include "sor_solid_tile.h"

using namespace sfl::host;

namespace sfl {
namespace host {
std::vector<uint8_t> solid_codes(const uint8_t *mask, int dim_x, int dim_y, size_t members);   // solids.cpp
}  // namespace host
}  // namespace sfl

namespace {

// item 4 on the velocity held; inside a step (item 3) the solid cells' velocity is zeroed by the same pass
int divergence_pass(sfl_context *c, float dx, bool zero_solids)
{
    SFL_TRY(ensure_field(c, SFL_FIELD_VELOCITY));
    SFL_TRY(ensure_field(c, SFL_FIELD_DIVERGENCE));
    SFL_TRY(use_device(c));
    const float two_dx_inv = 1.0f / (2.0f * dx);  // finitediff.cpp:36
    HIP_TRY(sfl::launch_solid_divergence(c->stream, c->div, c->vel, c->solids.d_codes, c->dim_x, c->gdim_y, two_dx_inv, zero_solids));
    if (zero_solids) ++c->vel_epoch;
    return SFL_OK;
}

int divergence(sfl_context *c, float dx) { return divergence_pass(c, dx, false); }

// item 5: ceil(iters / kD) launches of the tile kernel between p and its ping-pong partner, which the host swaps behind
// each; the first launch of a solve from zero reads no pressure at all.  SFL_OPT_SOR_FOLD has no say: the masked
// kernel knows only the rule's arithmetic.
int solve(sfl_context *c, float dx, int iters, float omega, bool warm)
{
    if (iters < 0) return fail(SFL_ERR_INVALID, "iters must be >= 0 (got %d)", iters);
    SFL_TRY(ensure_field(c, SFL_FIELD_DIVERGENCE));
    SFL_TRY(ensure_field(c, SFL_FIELD_PRESSURE));
    SFL_TRY(use_device(c));
    c->last_halo = c->last_launches = c->last_exchanges = 0;
    c->last_fuse = 2 * std::min(iters, sfl::solid_tile::kD);
    c->p_ghost_valid = 0;
    if (iters == 0) {   // a solve from zero leaves p = 0; a continued one the pressure as it is
        if (!warm) HIP_TRY(hipMemsetAsync(c->p, 0, c->local_cells() * sizeof(float), c->stream));
        return SFL_OK;
    }
    sfl::SorParams prm = sor_params(c, dx, omega);
    prm.fold = 0;
    const int launches = sfl::solid_tile::launches_of(iters);
    for (int l = 0; l < launches; ++l) {
        const int k = sfl::solid_tile::iterations_of_launch(iters, l);
        HIP_TRY(sfl::launch_solid_sor(c->stream, c->p_alt, l == 0 && !warm ? nullptr : c->p, c->div, c->solids.d_codes, c->dim_x, c->gdim_y, k, prm));
        std::swap(c->p, c->p_alt);
        ++c->last_launches;
    }
    return SFL_OK;
}

int gradient(sfl_context *c, float dx)
{
    SFL_TRY(ensure_field(c, SFL_FIELD_VELOCITY));
    SFL_TRY(ensure_field(c, SFL_FIELD_PRESSURE));
    SFL_TRY(use_device(c));
    const float two_dx_inv = 1.0f / (2.0f * dx);  // finitediff.cpp:78-79
    HIP_TRY(sfl::launch_solid_gradient(c->stream, c->vel, c->p, c->solids.d_codes, c->dim_x, c->gdim_y, two_dx_inv));
    ++c->vel_epoch;
    c->v_ghost_valid = 0;
    return SFL_OK;
}

int norm(sfl_context *c, float dx, unsigned *d_word)
{
    HIP_TRY(sfl::launch_solid_update_norm(c->stream, d_word, c->p, c->div, c->solids.d_codes, c->dim_x, c->gdim_y, dx));
    return SFL_OK;
}

int max_div(sfl_context *c, float two_dx_inv, unsigned *d_word)
{
    HIP_TRY(sfl::launch_solid_max_divergence(c->stream, d_word, c->vel, c->solids.d_codes, c->dim_x, c->gdim_y, two_dx_inv));
    return SFL_OK;
}

// One step by the rule (items 1 - 7), behind sfl_step's checks: one unfused sequence -- the existing velocity advection,
// the existing forces, the masked divergence (which also zeroes the solid cells' velocity), the masked solve, the masked
// gradient, the existing dye advection.  No seam, no small-grid one-launch step.
int step(sfl_context *c, float dt, float dx, int iters, float omega)
{
    SFL_TRY(sfl_advect_velocity(c, dt, 1));     // item 1
    SFL_TRY(apply_queued_forces(c));            // item 2
    SFL_TRY(divergence_pass(c, dx, true));      // items 3 and 4
    SFL_TRY(solve(c, dx, iters, omega, false)); // item 5
    SFL_TRY(gradient(c, dx));                   // item 6
    SFL_TRY(sfl_advect_color(c, dt, 0));        // item 7
    return SFL_OK;
}

void set_hooks(sfl_context *c)
{
    const bool on = c->solids.set;
    c->solids.step = on ? step : nullptr;
    c->solids.divergence = on ? divergence : nullptr;
    c->solids.solve = on ? solve : nullptr;
    c->solids.gradient = on ? gradient : nullptr;
    c->solids.norm = on ? norm : nullptr;
    c->solids.max_div = on ? max_div : nullptr;
    c->solids.rehook = on ? set_hooks : nullptr;
}

}  // namespace

extern "C" {

int sfl_set_solids(sfl_context *c, const uint8_t *mask)
{
    const char *call = "sfl_set_solids";
    if (!c) return fail(SFL_ERR_INVALID, "%s: ctx is NULL", call);
    if (mask && c->nranks != 1)
        return fail(SFL_ERR_STATE, "%s: whole-domain contexts only (slab %d/%d): a slab's exchanges and its kernels do not know solid cells; "
                    "nothing set", call, c->rank, c->nranks);
    if (mask && c->transport)
        return fail(SFL_ERR_STATE, "%s: the context has a transport attached, whose exchanges do not know solid cells: nothing set", call);
    HIP_TRY(hipSetDevice(c->device));
    ContextSolids &s = c->solids;
    if (!mask) {   // clear: the calls launch what they launched before; launches in flight may still read the bytes
        if (s.d_codes) {
            HIP_TRY(hipStreamSynchronize(c->stream));
            (void)hipFree(s.d_codes);
        }
        s = ContextSolids{};
        if (c->walls.drop) c->walls.drop(c);   // (a wall is a solid cell: the table goes with the mask)
        if (c->openings.restage) SFL_TRY(c->openings.restage(c));   // (the openings' bytes and pointers: every cell is fluid again)
        return SFL_OK;
    }
    const size_t bytes = (size_t)c->dim_x * (size_t)c->gdim_y;
    const std::vector<uint8_t> codes = solid_codes(mask, c->dim_x, c->gdim_y, 1);
    int64_t solid = 0;
    for (uint8_t b : codes) solid += b == 0;
    HIP_TRY(hipStreamSynchronize(c->stream));   // launches in flight may still read the bytes this call replaces
    if (!s.d_codes) {
        s = ContextSolids{};   // no solids unless the bytes are there
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
    set_hooks(c);
    HIP_TRY(hipMemcpyAsync(s.d_codes, codes.data(), bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));   // (`codes` goes with this call)
    s.set = true;
    s.solid_cells = solid;
    set_hooks(c);
    if (c->walls.drop) c->walls.drop(c);   // (the table was checked against the mask this call replaced: it goes)
    if (c->openings.restage) SFL_TRY(c->openings.restage(c));   // (an opening counts only where the cell is fluid)
    return SFL_OK;
}

int sfl_solids_info(sfl_context *c, int *set, int64_t *solid_cells)
{
    if (!c) return fail(SFL_ERR_INVALID, "sfl_solids_info: ctx is NULL");
    if (set) *set = c->solids.set ? 1 : 0;
    if (solid_cells) *solid_cells = c->solids.set ? c->solids.solid_cells : 0;
    return SFL_OK;
}

int sfl_solids_download(sfl_context *c, uint8_t *host, size_t bytes)
{
    const char *call = "sfl_solids_download";
    if (!c) return fail(SFL_ERR_INVALID, "%s: ctx is NULL", call);
    const size_t want = (size_t)c->dim_x * (size_t)c->gdim_y;
    if (bytes != want) return fail(SFL_ERR_INVALID, "%s: the mask of %d x %d cells is %zu bytes, got %zu", call, c->dim_x, c->gdim_y, want, bytes);
    if (!host) return fail(SFL_ERR_INVALID, "%s: host is NULL", call);
    if (!c->solids.set) {   // no solid cell anywhere
        memset(host, 0, bytes);
        return SFL_OK;
    }
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(host, c->solids.d_codes, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (size_t k = 0; k < bytes; ++k) host[k] = (host[k] & 16) ? 0 : 1;   // solid = not fluid
    return SFL_OK;
}

}  // extern "C"
