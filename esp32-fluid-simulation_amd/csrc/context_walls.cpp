// context_walls.cpp -- the wall velocities of a whole-domain context (include/sfl.h "WALL VELOCITIES";
// sfl_set_wall_velocity, _wall_velocity_info, _wall_velocity_download): the records checked against the mask that is set,
// duplicates removed, kept on the host in cell order (wall_table.h) and as a compact list on the device; the step a
// context runs while a table is held, with the two launches of context_walls.hip.  Host C++ only.
//
// The step and sfl_set_solids live in units that do not call into this one: what a context holds of its walls is plain
// data on the struct (context.h ContextWalls; sfl_destroy frees the list), and the two places that must know a table --
// the step and a change of the mask -- reach it through two pointers set here while a table is held and null otherwise:
// then every call launches exactly what it launched before there were walls.
#include "context.h"
#include "wall_kernels.h"

#include <cmath>

using namespace sfl::host;

namespace {

namespace wt = sfl::walls;

// item 8: the walls hold their velocity again
int scatter(sfl_context *c)
{
    SFL_TRY(use_device(c));
    HIP_TRY(sfl::launch_wall_scatter(c->stream, c->vel, c->walls.d_cells, c->walls.d_vel, (int)c->walls.row.size()));
    ++c->vel_epoch;
    c->v_ghost_valid = 0;
    return SFL_OK;
}

// One step with a wall table, behind sfl_step's checks.  Without item 3a the extended item 3 cannot be observed: the step
// that would have run -- the solids', or the openings' behind the same pointer -- runs as it is, and item 8 behind it.
// With item 3a: the viscous step's own sequence (context_viscous.cpp's step, restated: the two are kept in step by hand), with
// ONE launch in front of the diffusion that writes (0, 0) to every solid cell and the records to theirs, and the diffusion
// then called as the call of its own runs it: it reads a solid cell as it is.
int step(sfl_context *c, float dt, float dx, int iters, float omega)
{
    if (!c->viscosity.set) {
        SFL_TRY(c->solids.step(c, dt, dx, iters, omega));                                    // items 1 - 7
        return scatter(c);                                                                   // item 8
    }
    SFL_TRY(sfl_advect_velocity(c, dt, 1));                                                  // item 1
    SFL_TRY(apply_queued_forces(c));                                                         // item 2
    SFL_TRY(use_device(c));
    HIP_TRY(sfl::launch_wall_impose(c->stream, c->vel, c->solids.d_codes, (size_t)c->dim_x * (size_t)c->gdim_y, c->walls.d_cells, c->walls.d_vel,
                                    (int)c->walls.row.size()));                              // item 3, extended
    ++c->vel_epoch;
    c->v_ghost_valid = 0;
    SFL_TRY(sfl_diffuse_velocity(c, c->viscosity.nu, dt, dx, c->viscosity.sweeps));          // item 3a
    SFL_TRY(sfl_calculate_divergence(c, dx));                                                // item 4
    SFL_TRY(sfl_poisson_solve(c, dx, iters, omega));                                         // item 5
    SFL_TRY(sfl_subtract_gradient(c, dx));                                                   // item 6
    SFL_TRY(sfl_advect_color(c, dt, 0));                                                     // item 7
    return scatter(c);                                                                       // item 8
}

// the table goes: its list, its records, its two pointers.  The stream is idle.
void drop(sfl_context *c)
{
    if (c->walls.d_list) (void)hipFree(c->walls.d_list);
    c->walls = ContextWalls{};
}

size_t round8(size_t n) { return (n + 7) & ~(size_t)7; }

}  // namespace

extern "C" {

int sfl_set_wall_velocity(sfl_context *c, const int *cells_ij, const float *vel_xy, int n)
{
    const char *call = "sfl_set_wall_velocity";
    if (n < 0) return fail(SFL_ERR_INVALID, "%s: n must be >= 0 (got %d)", call, n);
    if (n > 0 && !cells_ij) return fail(SFL_ERR_INVALID, "%s: cells_ij is NULL with n = %d", call, n);
    if (n > 0 && !vel_xy) return fail(SFL_ERR_INVALID, "%s: vel_xy is NULL with n = %d", call, n);
    for (int k = 0; k < n; ++k)   // (needs no context: it answers on a box without a GPU too)
        if (!std::isfinite(vel_xy[2 * k]) || !std::isfinite(vel_xy[2 * k + 1]))
            return fail(SFL_ERR_INVALID, "%s: the velocity of a record must be finite (record %d: (%g, %g))", call, k, (double)vel_xy[2 * k],
                        (double)vel_xy[2 * k + 1]);
    if (!c) return fail(SFL_ERR_INVALID, "%s: ctx is NULL", call);
    ContextWalls &w = c->walls;
    if (n == 0) {   // clear: the steps launch what they launched before
        if (!w.on) return SFL_OK;
        SFL_TRY(use_device(c));
        HIP_TRY(hipStreamSynchronize(c->stream));   // launches in flight may still read the list
        drop(c);
        return SFL_OK;
    }
    if (!c->solids.set)
        return fail(SFL_ERR_STATE, "%s: the context has no solids set, and a wall is a solid cell: nothing set; set a mask first (sfl_set_solids)", call);
    // the records against the mask: inside the grid, and solid
    const int dim_x = c->dim_x, dim_y = c->gdim_y;
    const size_t cells = (size_t)dim_x * (size_t)dim_y;
    SFL_TRY(use_device(c));
    HIP_TRY(hipStreamSynchronize(c->stream));   // launches in flight may still read the list this call replaces
    std::vector<uint8_t> codes(cells);
    HIP_TRY(hipMemcpy(codes.data(), c->solids.d_codes, cells, hipMemcpyDeviceToHost));
    const wt::Offence bad = wt::first_offence(nullptr, cells_ij, n, dim_x, dim_y, codes.data(), false, 1);
    if (bad.kind == wt::Offence::kOutside)
        return fail(SFL_ERR_INVALID, "%s: record %d names cell (%d, %d), which is not inside the grid of %d x %d", call, bad.record, bad.i, bad.j, dim_x,
                    dim_y);
    if (bad.kind == wt::Offence::kFluid)
        return fail(SFL_ERR_INVALID, "%s: record %d names cell (%d, %d), which is not solid in the mask", call, bad.record, bad.i, bad.j);
    wt::Rows rows = wt::rows_of(nullptr, cells_ij, vel_xy, n, dim_x, 1);
    const wt::Table t = wt::table_of(rows, 1);
    // the list: the cells, behind them the velocities; allocated if it must grow, copied, and only then the context's pointers change
    const size_t at_vel = round8(t.cells.size() * sizeof(uint32_t)), want = at_vel + t.vel.size() * sizeof(float);
    std::vector<char> image(want, 0);
    memcpy(image.data(), t.cells.data(), t.cells.size() * sizeof(uint32_t));
    memcpy(image.data() + at_vel, t.vel.data(), t.vel.size() * sizeof(float));
    char *mem = static_cast<char *>(w.d_list);
    if (want > w.d_bytes) {
        void *fresh = nullptr;
        const hipError_t e = hipMalloc(&fresh, want);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(e == hipErrorOutOfMemory ? SFL_ERR_NOMEM : SFL_ERR_HIP, "%s: hipMalloc of %zu bytes of the wall table failed: %s", call, want,
                        hipGetErrorString(e));
        }
        mem = static_cast<char *>(fresh);
    }
    const hipError_t e = hipMemcpy(mem, image.data(), want, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (mem != w.d_list) (void)hipFree(mem);
        return fail(SFL_ERR_HIP, "%s: the copy of the wall table failed: %s", call, hipGetErrorString(e));
    }
    if (mem != w.d_list) {
        if (w.d_list) (void)hipFree(w.d_list);
        w.d_list = mem;
        w.d_bytes = want;
    }
    w.d_cells = reinterpret_cast<const uint32_t *>(mem);
    w.d_vel = reinterpret_cast<const float *>(mem + at_vel);
    w.row.swap(rows[0]);
    w.on = true;
    w.step = step;
    w.drop = drop;
    return SFL_OK;
}

int sfl_wall_velocity_info(sfl_context *c, int *records)
{
    if (!c) return fail(SFL_ERR_INVALID, "sfl_wall_velocity_info: ctx is NULL");
    if (records) *records = c->walls.on ? (int)c->walls.row.size() : 0;
    return SFL_OK;
}

int sfl_wall_velocity_download(sfl_context *c, int *cells_ij, float *vel_xy, int capacity)
{
    const char *call = "sfl_wall_velocity_download";
    if (!c) return fail(SFL_ERR_INVALID, "%s: ctx is NULL", call);
    if (capacity < 0) return fail(SFL_ERR_INVALID, "%s: capacity must be >= 0 (got %d)", call, capacity);
    const ContextWalls &w = c->walls;
    const size_t n = w.on ? w.row.size() : 0;
    if ((size_t)capacity < n) return fail(SFL_ERR_INVALID, "%s: the table holds %zu records, the arrays have room for %d", call, n, capacity);
    if (n == 0) return SFL_OK;
    if (!cells_ij || !vel_xy) return fail(SFL_ERR_INVALID, "%s: %s is NULL", call, cells_ij ? "vel_xy" : "cells_ij");
    for (size_t k = 0; k < n; ++k) {
        cells_ij[2 * k] = (int)(w.row[k].cell % (uint32_t)c->dim_x);
        cells_ij[2 * k + 1] = (int)(w.row[k].cell / (uint32_t)c->dim_x);
        vel_xy[2 * k] = w.row[k].u;
        vel_xy[2 * k + 1] = w.row[k].v;
    }
    return SFL_OK;
}

}  // extern "C"
