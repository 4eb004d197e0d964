// walls.cpp -- the wall velocities of a batch (include/sfl.h "WALL VELOCITIES"; sfl_batch_set_wall_velocity,
// _wall_velocity_info, _wall_velocity_download): the records checked against the mask that is set, duplicates removed, kept
// on the host in cell order (wall_table.h) and laid out as one CSR table on the device; the launches of batch_walls.hip
// that every step of batch.cpp makes while a table is held.  Host C++ only.
//
// batch.cpp and solids.cpp do not call into this unit: what a batch holds of its walls is plain data on the struct
// (batch_state.h Walls; freed by the destroy path), and the two places that must know a table -- the step and a change of
// the mask -- reach it through two pointers set here while a table is held and null otherwise: then a batch launches
// exactly what it launched before there were walls.
#include "batch_state.h"
#include "viscous_kernels.h"

#include <cmath>

using sfl::host::fail;

namespace {

namespace wt = sfl::walls;

// one step is due: the kernel on open codes where openings are set (with the profile's table where one is held), else the
// one on the solids' bytes (with the viscosity's records where one is set)
int step(sfl_batch *b, bool each, const sfl::BatchStep &a)
{
    const sfl::BatchProfile &walls = b->walls.table;
    if (b->openings.set) {
        const sfl_batch::Openings &o = b->openings;
        const sfl::BatchOpenings open{o.d_codes, o.codes_per_member ? b->cells : 0, o.d_inflow};
        const sfl::BatchProfile profile = o.profile_on ? o.profile_table : sfl::BatchProfile{nullptr, nullptr, nullptr};
        if (each)
            HIP_TRY(sfl::launch_batch_open_wall_step_each(b->stream, a, open, profile, walls, b->batch, b->d_members, b->d_report));
        else
            HIP_TRY(sfl::launch_batch_open_wall_step(b->stream, a, open, profile, walls, b->batch));
        return SFL_OK;
    }
    const sfl::BatchSolids solids{b->solids.d_codes, b->solids.per_member ? b->cells : 0};
    const sfl::BatchViscous *visc = b->viscosity.set ? static_cast<const sfl::BatchViscous *>(b->viscosity.d_table) : nullptr;
    if (each)
        HIP_TRY(sfl::launch_batch_wall_step_each(b->stream, a, solids, visc, walls, b->batch, b->d_members, b->d_report));
    else
        HIP_TRY(sfl::launch_batch_wall_step(b->stream, a, solids, visc, walls, b->batch));
    return SFL_OK;
}

// the table goes: its device memory, its rows, its two pointers.  The stream is idle.
void drop(sfl_batch *b)
{
    sfl_batch::Walls &w = b->walls;
    if (w.d_table) (void)hipFree(w.d_table);
    w = sfl_batch::Walls{};
}

size_t round8(size_t n) { return (n + 7) & ~(size_t)7; }

// The table of `rows` onto the device: built whole on the host, allocated if it must grow, copied; only then the batch's
// pointers change -- a failure leaves the table that was there.  The stream is idle.
int stage_table(sfl_batch *b, const wt::Rows &rows, const char *call)
{
    sfl_batch::Walls &w = b->walls;
    const wt::Table t = wt::table_of(rows, b->batch);
    if (!t.ok) return fail(SFL_ERR_INVALID, "%s: more than 2^31 - 1 records over all members", call);
    const size_t at_cells = round8(t.offsets.size() * sizeof(int)), at_vel = at_cells + round8(t.cells.size() * sizeof(uint32_t));
    const size_t want = at_vel + t.vel.size() * sizeof(float);
    std::vector<char> image(want, 0);
    memcpy(image.data(), t.offsets.data(), t.offsets.size() * sizeof(int));
    if (!t.cells.empty()) {
        memcpy(image.data() + at_cells, t.cells.data(), t.cells.size() * sizeof(uint32_t));
        memcpy(image.data() + at_vel, t.vel.data(), t.vel.size() * sizeof(float));
    }
    char *mem = static_cast<char *>(w.d_table);
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
        if (mem != w.d_table) (void)hipFree(mem);
        return fail(SFL_ERR_HIP, "%s: the copy of the wall table failed: %s", call, hipGetErrorString(e));
    }
    if (mem != w.d_table) {
        if (w.d_table) (void)hipFree(w.d_table);
        w.d_table = mem;
        w.d_bytes = want;
    }
    w.table = sfl::BatchProfile{reinterpret_cast<const int *>(mem), reinterpret_cast<const uint32_t *>(mem + at_cells),
                                reinterpret_cast<const float *>(mem + at_vel)};
    return SFL_OK;
}

}  // namespace

extern "C" {

int sfl_batch_set_wall_velocity(sfl_batch *b, const int *members, const int *cells_ij, const float *vel_xy, int n)
{
    const char *call = "sfl_batch_set_wall_velocity";
    if (n < 0) return fail(SFL_ERR_INVALID, "%s: n must be >= 0 (got %d)", call, n);
    if (n > 0 && !cells_ij) return fail(SFL_ERR_INVALID, "%s: cells_ij is NULL with n = %d", call, n);
    if (n > 0 && !vel_xy) return fail(SFL_ERR_INVALID, "%s: vel_xy is NULL with n = %d", call, n);
    for (int k = 0; k < n; ++k)   // (needs no batch: it answers on a box without a GPU too)
        if (!std::isfinite(vel_xy[2 * k]) || !std::isfinite(vel_xy[2 * k + 1]))
            return fail(SFL_ERR_INVALID, "%s: the velocity of a record must be finite (record %d: (%g, %g))", call, k, (double)vel_xy[2 * k],
                        (double)vel_xy[2 * k + 1]);
    if (!b) return fail(SFL_ERR_INVALID, "%s: batch is NULL", call);
    if (members)
        for (int k = 0; k < n; ++k)
            if (members[k] < 0 || members[k] >= b->batch)
                return fail(SFL_ERR_INVALID, "%s: record %d names member %d, which is not inside the batch's [0, %d)", call, k, members[k], b->batch);
    sfl_batch::Walls &w = b->walls;
    if (n == 0) {   // clear: the steps launch what they launched before
        if (!w.on) return SFL_OK;
        HIP_TRY(hipSetDevice(b->device));
        HIP_TRY(hipStreamSynchronize(b->stream));   // launches in flight may still read the table
        drop(b);
        return SFL_OK;
    }
    if (!b->solids.set)
        return fail(SFL_ERR_STATE, "%s: the batch has no solids set, and a wall is a solid cell: nothing set; set a mask first (sfl_batch_set_solids)",
                    call);
    // the records against the mask: inside the grid, and solid in the mask of every member they apply to
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(b->stream));   // launches in flight may still read the table this call replaces
    const bool per_member = b->solids.per_member;
    std::vector<uint8_t> codes(per_member ? (size_t)b->batch * b->cells : b->cells);
    HIP_TRY(hipMemcpy(codes.data(), b->solids.d_codes, codes.size(), hipMemcpyDeviceToHost));
    const wt::Offence bad = wt::first_offence(members, cells_ij, n, b->dim_x, b->dim_y, codes.data(), per_member, b->batch);
    if (bad.kind == wt::Offence::kOutside)
        return fail(SFL_ERR_INVALID, "%s: record %d names cell (%d, %d), which is not inside the grid of %d x %d", call, bad.record, bad.i, bad.j,
                    b->dim_x, b->dim_y);
    if (bad.kind == wt::Offence::kFluid) {
        if (per_member || members)
            return fail(SFL_ERR_INVALID, "%s: record %d names cell (%d, %d), which is not solid in the mask of member %d", call, bad.record, bad.i,
                        bad.j, bad.member);
        return fail(SFL_ERR_INVALID, "%s: record %d names cell (%d, %d), which is not solid in the mask", call, bad.record, bad.i, bad.j);
    }
    wt::Rows rows = wt::rows_of(members, cells_ij, vel_xy, n, b->dim_x, b->batch);
    SFL_TRY(stage_table(b, rows, call));
    w.rows.swap(rows);
    w.on = true;
    w.step = step;
    w.drop = drop;
    return SFL_OK;
}

int sfl_batch_wall_velocity_info(sfl_batch *b, int *set, int64_t *records)
{
    if (!b) return fail(SFL_ERR_INVALID, "sfl_batch_wall_velocity_info: batch is NULL");
    if (set) *set = b->walls.on ? 1 : 0;
    if (records) *records = b->walls.on ? wt::records_held(b->walls.rows, b->batch) : 0;
    return SFL_OK;
}

int sfl_batch_wall_velocity_download(sfl_batch *b, int member, int *cells_ij, float *vel_xy, int capacity, int *records)
{
    const char *call = "sfl_batch_wall_velocity_download";
    if (!b) return fail(SFL_ERR_INVALID, "%s: batch is NULL", call);
    if (member < 0 || member >= b->batch) return fail(SFL_ERR_INVALID, "%s: member %d is not inside the batch's [0, %d)", call, member, b->batch);
    if (capacity < 0) return fail(SFL_ERR_INVALID, "%s: capacity must be >= 0 (got %d)", call, capacity);
    const sfl_batch::Walls &w = b->walls;
    static const std::vector<wt::Record> none;
    const std::vector<wt::Record> &row = w.on ? w.rows[w.rows.size() == 1 ? 0 : (size_t)member] : none;
    if (records) *records = (int)row.size();
    if (capacity == 0 && !cells_ij && !vel_xy) return SFL_OK;   // the number alone
    if ((size_t)capacity < row.size())
        return fail(SFL_ERR_INVALID, "%s: member %d holds %zu records, the arrays have room for %d", call, member, row.size(), capacity);
    if (row.empty()) return SFL_OK;
    if (!cells_ij || !vel_xy) return fail(SFL_ERR_INVALID, "%s: %s is NULL", call, cells_ij ? "vel_xy" : "cells_ij");
    for (size_t k = 0; k < row.size(); ++k) {
        cells_ij[2 * k] = (int)(row[k].cell % (uint32_t)b->dim_x);
        cells_ij[2 * k + 1] = (int)(row[k].cell / (uint32_t)b->dim_x);
        vel_xy[2 * k] = row[k].u;
        vel_xy[2 * k + 1] = row[k].v;
    }
    return SFL_OK;
}

}  // extern "C"
