// context_openings.cpp -- inflow and outflow cells on the rim of a whole-domain context (include/sfl.h "OPENINGS OF A CONTEXT";
// sfl_set_openings, _set_inflow, _openings_info, _openings_download): the user's map checked (openings.cpp check_open_map),
// turned with the solids' code bytes as they stand into two bytes per cell and a compact list of the fluid inflow cells, kept
// on the device, and the launches of context_openings.hip that the step, the operators, the solves, the update norm, the
// statistics and the history's sample make while a map is set; and the context's inflow profile and flux record (include/sfl.h
// "INFLOW PROFILES AND FLUX": sfl_set_inflow_profile, _inflow_profile_info, _inflow_profile_download, sfl_openings_flux; the
// kernels of inflow.hip).  Host C++ only.
//
// Those calls reach the masked launches through the six pointers of ContextSolids (context.h).  While openings are set this
// unit puts its own functions there, and takes them out again when the map is cleared -- the solids' unit then puts its own
// back or leaves them null: no call site knows openings, and with none set every call launches exactly what it launched
// before.  ContextSolids::set and ::d_codes are the solids' alone: sfl_solids_info, the loads and the viscous kernels see what
// they saw before.
#include "context.h"
#include "open_kernels.h"
#include "sor_open_tile.h"

#include <cmath>

using namespace sfl::host;

namespace sfl {
namespace host {
std::vector<uint8_t> solid_codes(const uint8_t *mask, int dim_x, int dim_y, size_t members);                       // solids.cpp
int open_side(int i, int j, int dim_x, int dim_y);                                                                  // openings.cpp
bool check_open_map(const uint8_t *open, int dim_x, int dim_y, size_t members, char *why, size_t why_bytes);        // openings.cpp
}  // namespace host
}  // namespace sfl

namespace {

int divergence_pass(sfl_context *c, float dx, bool zero_solids)
{
    SFL_TRY(ensure_field(c, SFL_FIELD_VELOCITY));
    SFL_TRY(ensure_field(c, SFL_FIELD_DIVERGENCE));
    SFL_TRY(use_device(c));
    const float two_dx_inv = 1.0f / (2.0f * dx);  // finitediff.cpp:36
    HIP_TRY(sfl::launch_open_divergence(c->stream, c->div, c->vel, c->openings.d_codes, c->openings.d_open, c->dim_x, c->gdim_y, two_dx_inv, zero_solids));
    if (zero_solids) ++c->vel_epoch;
    return SFL_OK;
}

int divergence(sfl_context *c, float dx) { return divergence_pass(c, dx, false); }

// item 5 as context_solids.cpp runs it: ceil(iters / kD) launches between p and its ping-pong partner
int solve(sfl_context *c, float dx, int iters, float omega, bool warm)
{
    if (iters < 0) return fail(SFL_ERR_INVALID, "iters must be >= 0 (got %d)", iters);
    SFL_TRY(ensure_field(c, SFL_FIELD_DIVERGENCE));
    SFL_TRY(ensure_field(c, SFL_FIELD_PRESSURE));
    SFL_TRY(use_device(c));
    c->last_halo = c->last_launches = c->last_exchanges = 0;
    c->last_fuse = 2 * std::min(iters, sfl::solid_tile::kD);
    c->p_ghost_valid = 0;
    if (iters == 0) {
        if (!warm) HIP_TRY(hipMemsetAsync(c->p, 0, c->local_cells() * sizeof(float), c->stream));
        return SFL_OK;
    }
    sfl::SorParams prm = sor_params(c, dx, omega);
    prm.fold = 0;
    const int launches = sfl::solid_tile::launches_of(iters);
    for (int l = 0; l < launches; ++l) {
        const int k = sfl::solid_tile::iterations_of_launch(iters, l);
        HIP_TRY(sfl::launch_open_sor(c->stream, c->p_alt, l == 0 && !warm ? nullptr : c->p, c->div, c->openings.d_codes, c->openings.d_open, c->dim_x,
                                     c->gdim_y, k, prm));
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
    HIP_TRY(sfl::launch_open_gradient(c->stream, c->vel, c->p, c->openings.d_codes, c->openings.d_open, c->dim_x, c->gdim_y, two_dx_inv));
    ++c->vel_epoch;
    c->v_ghost_valid = 0;
    return SFL_OK;
}

int norm(sfl_context *c, float dx, unsigned *d_word)
{
    HIP_TRY(sfl::launch_open_update_norm(c->stream, d_word, c->p, c->div, c->openings.d_codes, c->openings.d_open, c->dim_x, c->gdim_y, dx));
    return SFL_OK;
}

int max_div(sfl_context *c, float two_dx_inv, unsigned *d_word)
{
    HIP_TRY(sfl::launch_open_max_divergence(c->stream, d_word, c->vel, c->openings.d_codes, c->openings.d_open, c->dim_x, c->gdim_y, two_dx_inv));
    return SFL_OK;
}

// One step by the rule, behind sfl_step's checks: the unfused sequence of context_solids.cpp with item 2a behind the forces.
// The operators above never impose the inflow.
int step(sfl_context *c, float dt, float dx, int iters, float omega)
{
    SFL_TRY(sfl_advect_velocity(c, dt, 1));     // item 1
    SFL_TRY(apply_queued_forces(c));            // item 2
    SFL_TRY(use_device(c));
    if (c->openings.profile_on)                 // item 2a, with a profile: one velocity per list entry
        HIP_TRY(sfl::launch_open_inflow_profile(c->stream, c->vel, c->openings.d_inflow_cells, c->openings.d_inflow_values, (int)c->openings.inflow_cells));
    else
        HIP_TRY(sfl::launch_open_inflow(c->stream, c->vel, c->openings.d_inflow_cells, (int)c->openings.inflow_cells, c->openings.inflow[0],
                                        c->openings.inflow[1]));   // item 2a
    SFL_TRY(divergence_pass(c, dx, true));      // items 3 and 4
    SFL_TRY(solve(c, dx, iters, omega, false)); // item 5
    SFL_TRY(gradient(c, dx));                   // item 6
    SFL_TRY(sfl_advect_color(c, dt, 0));        // item 7
    return SFL_OK;
}

void take_hooks(sfl_context *c)
{
    ContextSolids &s = c->solids;
    s.step = step;
    s.divergence = divergence;
    s.solve = solve;
    s.gradient = gradient;
    s.norm = norm;
    s.max_div = max_div;
}

int restage(sfl_context *c);

void free_arrays(ContextOpenings &o)
{
    for (void *m : {(void *)o.d_codes, (void *)o.d_open, (void *)o.d_inflow_cells, (void *)o.d_inflow_values, o.d_flux})
        if (m) (void)hipFree(m);
    o.d_codes = o.d_open = nullptr;
    o.d_inflow_cells = nullptr;
    o.d_inflow_values = nullptr;
    o.d_flux = nullptr;
}

int device_array(void **mem, size_t bytes, const char *call)
{
    const hipError_t e = hipMalloc(mem, bytes ? bytes : 1);
    if (e == hipSuccess) return SFL_OK;
    (void)hipGetLastError();
    *mem = nullptr;
    return fail(e == hipErrorOutOfMemory ? SFL_ERR_NOMEM : SFL_ERR_HIP, "%s: hipMalloc of %zu bytes failed: %s", call, bytes, hipGetErrorString(e));
}

// The velocities of a profile beside the compact list ("INFLOW PROFILES AND FLUX"): for list entry k the velocity of `profile`'s
// record on that cell where it has one, the uniform inflow elsewhere -- both are in cell order.  Allocated afresh (the list's
// length follows the mask) and copied; only then the context's pointer changes.  The stream is idle.
int stage_values(sfl_context *c, const std::vector<ContextOpenings::ProfileRecord> &profile, const char *call)
{
    ContextOpenings &o = c->openings;
    std::vector<float> values(2 * o.list.size());
    size_t r = 0;
    for (size_t k = 0; k < o.list.size(); ++k) {
        while (r < profile.size() && profile[r].cell < o.list[k]) ++r;   // (a record on a solid inflow cell is not in the list)
        const bool named = r < profile.size() && profile[r].cell == o.list[k];
        values[2 * k] = named ? profile[r].u : o.inflow[0];
        values[2 * k + 1] = named ? profile[r].v : o.inflow[1];
    }
    void *mem = nullptr;
    SFL_TRY(device_array(&mem, values.size() * sizeof(float), call));
    if (!values.empty()) {
        const hipError_t e = hipMemcpy(mem, values.data(), values.size() * sizeof(float), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(mem);
            return fail(SFL_ERR_HIP, "%s: the copy of the profile's velocities failed: %s", call, hipGetErrorString(e));
        }
    }
    if (o.d_inflow_values) (void)hipFree(o.d_inflow_values);
    o.d_inflow_values = static_cast<float *>(mem);
    return SFL_OK;
}

// The two bytes per cell and the list of inflow cells from the map held and the solids as they stand, onto the device; then
// the pointers.  On failure the openings are off and hold nothing.
int stage(sfl_context *c, const char *call)
{
    ContextOpenings &o = c->openings;
    const int dim_x = c->dim_x, dim_y = c->gdim_y;
    const size_t cells = (size_t)dim_x * (size_t)dim_y;
    HIP_TRY(hipStreamSynchronize(c->stream));   // launches in flight may still read the arrays this call replaces
    std::vector<uint8_t> codes(cells);
    if (c->solids.set) {
        HIP_TRY(hipMemcpyAsync(codes.data(), c->solids.d_codes, cells, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    } else {
        const std::vector<uint8_t> none(cells, 0);
        codes = solid_codes(none.data(), dim_x, dim_y, 1);
    }
    std::vector<uint8_t> open(cells, 0);
    std::vector<uint32_t> list;
    int64_t out = 0;
    for (int j = 0; j < dim_y; ++j)
        for (int i = 0; i < dim_x; ++i) {
            const size_t g = (size_t)j * dim_x + i;
            const int v = o.map[g];
            if (!v || !(codes[g] & 16)) continue;   // an opening counts only where the cell is fluid
            open[g] = (uint8_t)(open_side(i, j, dim_x, dim_y) | (v == SFL_OPEN_OUTFLOW ? sfl::open_tile::kOpenOutflow : 0));
            if (v == SFL_OPEN_OUTFLOW) ++out;
            else list.push_back((uint32_t)g);
        }
    if (!o.d_codes) {
        void *a = nullptr, *b = nullptr;
        SFL_TRY(device_array(&a, cells, call));
        o.d_codes = static_cast<uint8_t *>(a);
        if (device_array(&b, cells, call) != SFL_OK) {
            free_arrays(o);
            return SFL_ERR_NOMEM;
        }
        o.d_open = static_cast<uint8_t *>(b);
    }
    if (o.d_inflow_cells) (void)hipFree(o.d_inflow_cells);   // (the list's length follows the mask)
    void *l = nullptr;
    if (device_array(&l, list.size() * sizeof(uint32_t), call) != SFL_OK) {
        o.d_inflow_cells = nullptr;
        free_arrays(o);
        return SFL_ERR_NOMEM;
    }
    o.d_inflow_cells = static_cast<uint32_t *>(l);
    HIP_TRY(hipMemcpyAsync(o.d_codes, codes.data(), cells, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(o.d_open, open.data(), cells, hipMemcpyHostToDevice, c->stream));
    if (!list.empty()) HIP_TRY(hipMemcpyAsync(o.d_inflow_cells, list.data(), list.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));   // (the host arrays go with this call)
    o.inflow_cells = (int64_t)list.size();
    o.outflow_cells = out;
    o.list.swap(list);
    if (o.profile_on) SFL_TRY(stage_values(c, o.profile, call));   // (on failure the caller drops the openings, the profile with them)
    o.set = true;
    o.restage = restage;
    take_hooks(c);
    return SFL_OK;
}

// sfl_set_solids changed the mask and put its own pointers back: form the bytes again, take the pointers again
int restage(sfl_context *c)
{
    c->openings.set = false;
    const int rc = stage(c, "sfl_set_solids");
    if (rc != SFL_OK) {   // the openings are off: the mask is as set, the map is dropped
        free_arrays(c->openings);
        c->openings = ContextOpenings{};
    }
    return rc;
}

int check_inflow(const char *call, float x, float y)
{
    if (!std::isfinite(x) || !std::isfinite(y))
        return fail(SFL_ERR_INVALID, "%s: the inflow velocity must be finite (got (%g, %g))", call, (double)x, (double)y);
    return SFL_OK;
}

}  // namespace

extern "C" {

int sfl_set_openings(sfl_context *c, const uint8_t *open, float inflow_x, float inflow_y)
{
    const char *call = "sfl_set_openings";
    if (open) SFL_TRY(check_inflow(call, inflow_x, inflow_y));   // (needs no context: it answers on a box without a GPU too)
    if (!c) return fail(SFL_ERR_INVALID, "%s: ctx is NULL", call);
    if (open) {
        char why[200];
        if (!check_open_map(open, c->dim_x, c->gdim_y, 1, why, sizeof why)) return fail(SFL_ERR_INVALID, "%s: %s", call, why);
        if (c->nranks != 1)
            return fail(SFL_ERR_STATE, "%s: whole-domain contexts only (slab %d/%d): a slab's exchanges and its kernels do not know openings; "
                        "nothing set", call, c->rank, c->nranks);
        if (c->transport)
            return fail(SFL_ERR_STATE, "%s: the context has a transport attached, whose exchanges do not know openings: nothing set", call);
        if (c->viscosity.set)
            return fail(SFL_ERR_STATE, "%s: viscosity is set (sfl_set_viscosity) and the viscous kernels do not know openings: nothing set; "
                        "clear it first (sfl_set_viscosity(ctx, 0, 0))", call);
    }
    HIP_TRY(hipSetDevice(c->device));
    ContextOpenings &o = c->openings;
    if (!open) {   // clear: the pointers go back to what the solids alone make them
        if (!o.set) return SFL_OK;
        HIP_TRY(hipStreamSynchronize(c->stream));
        free_arrays(o);
        o = ContextOpenings{};
        c->solids.step = nullptr;
        c->solids.divergence = nullptr;
        c->solids.solve = nullptr;
        c->solids.gradient = nullptr;
        c->solids.norm = nullptr;
        c->solids.max_div = nullptr;
        if (c->solids.set && c->solids.rehook) c->solids.rehook(c);
        return SFL_OK;
    }
    o.map.assign(open, open + (size_t)c->dim_x * (size_t)c->gdim_y);
    o.profile.clear();   // a new map drops the inflow profile
    o.profile_on = false;
    o.inflow[0] = inflow_x;
    o.inflow[1] = inflow_y;
    const int rc = stage(c, call);
    if (rc != SFL_OK && !o.set) o.map.clear();
    return rc;
}

int sfl_set_inflow(sfl_context *c, float inflow_x, float inflow_y)
{
    const char *call = "sfl_set_inflow";
    SFL_TRY(check_inflow(call, inflow_x, inflow_y));
    if (!c) return fail(SFL_ERR_INVALID, "%s: ctx is NULL", call);
    if (!c->openings.set)
        return fail(SFL_ERR_STATE, "%s: the context has no openings set: nothing changed; set a map with its inflow first (sfl_set_openings)", call);
    if (c->openings.profile_on) {   // the cells the profile does not name hold the uniform inflow: the velocities are formed again
        ContextOpenings &o = c->openings;
        const float old[2] = {o.inflow[0], o.inflow[1]};
        SFL_TRY(use_device(c));
        HIP_TRY(hipStreamSynchronize(c->stream));   // launches in flight may still read the array this call replaces
        o.inflow[0] = inflow_x;
        o.inflow[1] = inflow_y;
        const int rc = stage_values(c, o.profile, call);
        if (rc != SFL_OK) {
            o.inflow[0] = old[0];
            o.inflow[1] = old[1];
        }
        return rc;
    }
    c->openings.inflow[0] = inflow_x;   // (a kernel argument of the next step: nothing to stage)
    c->openings.inflow[1] = inflow_y;
    return SFL_OK;
}

int sfl_openings_info(sfl_context *c, int *set, float *inflow_x, float *inflow_y, int64_t *inflow_cells, int64_t *outflow_cells)
{
    if (!c) return fail(SFL_ERR_INVALID, "sfl_openings_info: ctx is NULL");
    const ContextOpenings &o = c->openings;
    if (set) *set = o.set ? 1 : 0;
    if (inflow_x) *inflow_x = o.set ? o.inflow[0] : 0.0f;
    if (inflow_y) *inflow_y = o.set ? o.inflow[1] : 0.0f;
    if (inflow_cells) *inflow_cells = o.set ? o.inflow_cells : 0;
    if (outflow_cells) *outflow_cells = o.set ? o.outflow_cells : 0;
    return SFL_OK;
}

int sfl_openings_download(sfl_context *c, uint8_t *host, size_t bytes)
{
    const char *call = "sfl_openings_download";
    if (!c) return fail(SFL_ERR_INVALID, "%s: ctx is NULL", call);
    const size_t want = (size_t)c->dim_x * (size_t)c->gdim_y;
    if (bytes != want) return fail(SFL_ERR_INVALID, "%s: the map of %d x %d cells is %zu bytes, got %zu", call, c->dim_x, c->gdim_y, want, bytes);
    if (!host) return fail(SFL_ERR_INVALID, "%s: host is NULL", call);
    if (!c->openings.set) memset(host, 0, bytes);
    else memcpy(host, c->openings.map.data(), bytes);
    return SFL_OK;
}

// ---- the inflow profile and the flux (include/sfl.h "INFLOW PROFILES AND FLUX") -----------------------------------------------
int sfl_set_inflow_profile(sfl_context *c, const int *cells_ij, const float *vel_xy, int n)
{
    const char *call = "sfl_set_inflow_profile";
    if (n < 0) return fail(SFL_ERR_INVALID, "%s: n must be >= 0 (got %d)", call, n);
    if (n > 0 && !cells_ij) return fail(SFL_ERR_INVALID, "%s: cells_ij is NULL with n = %d", call, n);
    if (n > 0 && !vel_xy) return fail(SFL_ERR_INVALID, "%s: vel_xy is NULL with n = %d", call, n);
    for (int k = 0; k < n; ++k)   // (needs no context: it answers on a box without a GPU too)
        if (!std::isfinite(vel_xy[2 * k]) || !std::isfinite(vel_xy[2 * k + 1]))
            return fail(SFL_ERR_INVALID, "%s: the velocity of a record must be finite (record %d: (%g, %g))", call, k, (double)vel_xy[2 * k],
                        (double)vel_xy[2 * k + 1]);
    if (!c) return fail(SFL_ERR_INVALID, "%s: ctx is NULL", call);
    ContextOpenings &o = c->openings;
    if (n == 0) {   // clear: the uniform inflow's launch again
        if (!o.profile_on) return SFL_OK;
        SFL_TRY(use_device(c));
        HIP_TRY(hipStreamSynchronize(c->stream));   // launches in flight may still read the velocities
        if (o.d_inflow_values) (void)hipFree(o.d_inflow_values);
        o.d_inflow_values = nullptr;
        o.profile.clear();
        o.profile_on = false;
        return SFL_OK;
    }
    if (!o.set)
        return fail(SFL_ERR_STATE, "%s: the context has no openings set, and without openings there is no profile: nothing set; set a map with its "
                    "inflow first (sfl_set_openings)", call);
    const int dim_x = c->dim_x, dim_y = c->gdim_y;
    std::vector<ContextOpenings::ProfileRecord> rows;
    rows.reserve((size_t)n);
    for (int k = 0; k < n; ++k) {
        const int i = cells_ij[2 * k], j = cells_ij[2 * k + 1];
        if (i < 0 || i >= dim_x || j < 0 || j >= dim_y)
            return fail(SFL_ERR_INVALID, "%s: record %d names cell (%d, %d), which is not inside the grid of %d x %d", call, k, i, j, dim_x, dim_y);
        const size_t g = (size_t)j * dim_x + i;
        if (o.map[g] != SFL_OPEN_INFLOW)
            return fail(SFL_ERR_INVALID, "%s: record %d names cell (%d, %d), whose map byte is %d, not SFL_OPEN_INFLOW (1)", call, k, i, j, (int)o.map[g]);
        rows.push_back(ContextOpenings::ProfileRecord{(uint32_t)g, vel_xy[2 * k], vel_xy[2 * k + 1]});
    }
    std::stable_sort(rows.begin(), rows.end(), [](const ContextOpenings::ProfileRecord &a, const ContextOpenings::ProfileRecord &b) { return a.cell < b.cell; });
    size_t kept = 0;
    for (size_t k = 0; k < rows.size(); ++k) {   // of two records on one cell the later wins
        if (k + 1 < rows.size() && rows[k + 1].cell == rows[k].cell) continue;
        rows[kept++] = rows[k];
    }
    rows.resize(kept);
    SFL_TRY(use_device(c));
    HIP_TRY(hipStreamSynchronize(c->stream));   // launches in flight may still read the velocities this call replaces
    SFL_TRY(stage_values(c, rows, call));
    o.profile.swap(rows);
    o.profile_on = true;
    return SFL_OK;
}

int sfl_inflow_profile_info(sfl_context *c, int *records)
{
    if (!c) return fail(SFL_ERR_INVALID, "sfl_inflow_profile_info: ctx is NULL");
    if (records) *records = c->openings.set && c->openings.profile_on ? (int)c->openings.profile.size() : 0;
    return SFL_OK;
}

int sfl_inflow_profile_download(sfl_context *c, int *cells_ij, float *vel_xy, int capacity)
{
    const char *call = "sfl_inflow_profile_download";
    if (!c) return fail(SFL_ERR_INVALID, "%s: ctx is NULL", call);
    if (capacity < 0) return fail(SFL_ERR_INVALID, "%s: capacity must be >= 0 (got %d)", call, capacity);
    const ContextOpenings &o = c->openings;
    const size_t n = o.set && o.profile_on ? o.profile.size() : 0;
    if ((size_t)capacity < n) return fail(SFL_ERR_INVALID, "%s: the profile holds %zu records, the arrays have room for %d", call, n, capacity);
    if (n == 0) return SFL_OK;
    if (!cells_ij || !vel_xy) return fail(SFL_ERR_INVALID, "%s: %s is NULL", call, cells_ij ? "vel_xy" : "cells_ij");
    for (size_t k = 0; k < n; ++k) {
        cells_ij[2 * k] = (int)(o.profile[k].cell % (uint32_t)c->dim_x);
        cells_ij[2 * k + 1] = (int)(o.profile[k].cell / (uint32_t)c->dim_x);
        vel_xy[2 * k] = o.profile[k].u;
        vel_xy[2 * k + 1] = o.profile[k].v;
    }
    return SFL_OK;
}

int sfl_openings_flux(sfl_context *c, struct sfl_open_flux *out)
{
    const char *call = "sfl_openings_flux";
    if (!c) return fail(SFL_ERR_INVALID, "%s: ctx is NULL", call);
    if (!out) return fail(SFL_ERR_INVALID, "%s: out is NULL", call);
    ContextOpenings &o = c->openings;
    memset(out, 0, sizeof *out);
    if (!o.set || o.inflow_cells + o.outflow_cells == 0) return SFL_OK;   // nothing live: zeros, no launch
    SFL_TRY(ensure_field(c, SFL_FIELD_VELOCITY));
    SFL_TRY(use_device(c));
    if (!o.d_flux) SFL_TRY(device_array(&o.d_flux, sizeof *out, call));
    struct sfl_open_flux *d = static_cast<struct sfl_open_flux *>(o.d_flux);
    HIP_TRY(sfl::launch_open_flux(c->stream, d, c->vel, o.d_open, c->dim_x, c->gdim_y));
    HIP_TRY(hipMemcpyAsync(out, d, sizeof *out, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SFL_OK;
}

}  // extern "C"
