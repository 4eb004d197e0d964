// inflow.cpp -- the inflow profile of a batch and the flux through its openings (include/sfl.h "INFLOW PROFILES AND FLUX";
// sfl_batch_set_inflow_profile, _inflow_profile_info, _inflow_profile_download, sfl_batch_openings_flux): the records
// checked against the map held, duplicates removed, kept on the host in cell order, and turned with the open codes as they
// stand into one CSR table on the device that names only fluid inflow cells; the launches of the profile's step kernels
// (batch_openings.hip) and of the flux kernel (inflow.hip).  Host C++ only.
//
// openings.cpp does not call into this unit: what a batch holds of its profile is plain data on the struct (batch_state.h
// Openings; freed where the codes are), and the two places that must know a profile -- the openings' step and the staging
// of the codes behind a new mask -- reach it through two pointers set here while a profile is held and null otherwise:
// then a batch with openings launches exactly what it launched before there were profiles.
#include "batch_state.h"

#include <cmath>

using sfl::host::fail;

namespace {

typedef sfl_batch::Openings::ProfileRecord Record;
static_assert(sizeof(struct sfl_open_flux) == 40 && offsetof(struct sfl_open_flux, outflow) == 8 && offsetof(struct sfl_open_flux, exp2) == 16 &&
                  offsetof(struct sfl_open_flux, max_abs_n) == 20 && offsetof(struct sfl_open_flux, inflow_cells) == 24 &&
                  offsetof(struct sfl_open_flux, nonfinite) == 32 && offsetof(struct sfl_open_flux, reserved) == 36,
              "include/sfl.h: 40 bytes");

sfl::BatchOpenings openings_of(const sfl_batch *b)
{
    return sfl::BatchOpenings{b->openings.d_codes, b->openings.codes_per_member ? b->cells : 0, b->openings.d_inflow};
}

int profile_step(sfl_batch *b, bool each, const sfl::BatchStep &a)
{
    if (each)
        HIP_TRY(sfl::launch_batch_open_profile_step_each(b->stream, a, openings_of(b), b->openings.profile_table, b->batch, b->d_members, b->d_report));
    else
        HIP_TRY(sfl::launch_batch_open_profile_step(b->stream, a, openings_of(b), b->openings.profile_table, b->batch));
    return SFL_OK;
}

size_t round8(size_t n) { return (n + 7) & ~(size_t)7; }

// The table of the rows `rows` (one, or one per member) by the open codes `codes` (member stride `stride`, 0 = shared): the
// records on cells that are fluid inflow cells now, per member in cell order.  Built whole on the host, allocated if it must
// grow, copied; only then the batch's pointers change -- a failure leaves the table that was there.  The stream is idle.
int stage_table(sfl_batch *b, const std::vector<std::vector<Record>> &rows, bool shared, const uint16_t *codes, size_t stride, const char *call)
{
    sfl_batch::Openings &o = b->openings;
    const size_t members = (size_t)b->batch;
    std::vector<int> offsets(members + 1, 0);
    std::vector<uint32_t> cells;
    std::vector<float> vel;
    for (size_t m = 0; m < members; ++m) {
        const uint16_t *mine = codes + m * stride;
        for (const Record &r : rows[shared ? 0 : m]) {
            const int code = mine[r.cell];
            if (!(code >> 8 & 15) || (code & 1 << 12)) continue;   // (solid at the time: an opening counts only where the cell is fluid)
            cells.push_back(r.cell);
            vel.push_back(r.u);
            vel.push_back(r.v);
        }
        if (cells.size() > (size_t)INT32_MAX) return fail(SFL_ERR_INVALID, "%s: more than 2^31 - 1 records over all members", call);
        offsets[m + 1] = (int)cells.size();
    }
    const size_t at_cells = round8(offsets.size() * sizeof(int)), at_vel = at_cells + round8(cells.size() * sizeof(uint32_t));
    const size_t want = at_vel + vel.size() * sizeof(float);
    std::vector<char> image(want, 0);
    memcpy(image.data(), offsets.data(), offsets.size() * sizeof(int));
    if (!cells.empty()) {
        memcpy(image.data() + at_cells, cells.data(), cells.size() * sizeof(uint32_t));
        memcpy(image.data() + at_vel, vel.data(), vel.size() * sizeof(float));
    }
    char *mem = static_cast<char *>(o.d_profile);
    if (want > o.d_profile_bytes) {
        void *fresh = nullptr;
        const hipError_t e = hipMalloc(&fresh, want);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(e == hipErrorOutOfMemory ? SFL_ERR_NOMEM : SFL_ERR_HIP, "%s: hipMalloc of %zu bytes of the profile's table failed: %s", call,
                        want, hipGetErrorString(e));
        }
        mem = static_cast<char *>(fresh);
    }
    const hipError_t e = hipMemcpy(mem, image.data(), want, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (mem != o.d_profile) (void)hipFree(mem);
        return fail(SFL_ERR_HIP, "%s: the copy of the profile's table failed: %s", call, hipGetErrorString(e));
    }
    if (mem != o.d_profile) {
        if (o.d_profile) (void)hipFree(o.d_profile);
        o.d_profile = mem;
        o.d_profile_bytes = want;
    }
    o.profile_table = sfl::BatchProfile{reinterpret_cast<const int *>(mem), reinterpret_cast<const uint32_t *>(mem + at_cells),
                                        reinterpret_cast<const float *>(mem + at_vel)};
    return SFL_OK;
}

// openings.cpp has formed the codes again (a new mask): the table follows them
int profile_restage(sfl_batch *b, const uint16_t *codes, size_t member_stride)
{
    return stage_table(b, b->openings.profile, b->openings.profile_shared, codes, member_stride, "sfl_batch_set_solids");
}

// the profile goes: its table, its records, its two pointers (openings.cpp's drop_profile is the twin that a new map runs:
// that unit does not call into this one)
void drop(sfl_batch *b)
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

// the records of one row sorted by cell, of two on one cell the later kept
void unique_by_cell(std::vector<Record> &row)
{
    std::stable_sort(row.begin(), row.end(), [](const Record &a, const Record &b) { return a.cell < b.cell; });
    size_t n = 0;
    for (size_t k = 0; k < row.size(); ++k) {
        if (k + 1 < row.size() && row[k + 1].cell == row[k].cell) continue;
        row[n++] = row[k];
    }
    row.resize(n);
}

}  // namespace

extern "C" {

int sfl_batch_set_inflow_profile(sfl_batch *b, const int *members, const int *cells_ij, const float *vel_xy, int n)
{
    const char *call = "sfl_batch_set_inflow_profile";
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
    sfl_batch::Openings &o = b->openings;
    if (n == 0) {   // clear: the openings' own step again
        if (!o.profile_on) return SFL_OK;
        HIP_TRY(hipSetDevice(b->device));
        HIP_TRY(hipStreamSynchronize(b->stream));   // launches in flight may still read the table
        drop(b);
        return SFL_OK;
    }
    if (b->large)
        return fail(SFL_ERR_STATE, "%s: a batch of sfl_batch_create_large has no openings and so no inflow profile: nothing set", call);
    if (!o.set)
        return fail(SFL_ERR_STATE, "%s: the batch has no openings set, and without openings there is no profile: nothing set; set a map with its "
                    "inflow first (sfl_batch_set_openings)", call);
    // the records against the map: inside the grid, and SFL_OPEN_INFLOW in the map of every member they apply to
    const int dim_x = b->dim_x, dim_y = b->dim_y;
    for (int k = 0; k < n; ++k) {
        const int i = cells_ij[2 * k], j = cells_ij[2 * k + 1];
        if (i < 0 || i >= dim_x || j < 0 || j >= dim_y)
            return fail(SFL_ERR_INVALID, "%s: record %d names cell (%d, %d), which is not inside the grid of %d x %d", call, k, i, j, dim_x, dim_y);
        const size_t c = (size_t)j * dim_x + i;
        const int m0 = members ? members[k] : 0, m1 = members ? members[k] + 1 : (o.per_member ? b->batch : 1);
        for (int m = m0; m < m1; ++m) {
            const int byte = o.map[(o.per_member ? (size_t)m * b->cells : 0) + c];
            if (byte == SFL_OPEN_INFLOW) continue;
            if (o.per_member || members)
                return fail(SFL_ERR_INVALID, "%s: record %d names cell (%d, %d), whose map byte in member %d is %d, not SFL_OPEN_INFLOW (1)", call, k, i,
                            j, m, byte);
            return fail(SFL_ERR_INVALID, "%s: record %d names cell (%d, %d), whose map byte is %d, not SFL_OPEN_INFLOW (1)", call, k, i, j, byte);
        }
    }
    const bool shared = members == nullptr;
    std::vector<std::vector<Record>> rows(shared ? 1 : (size_t)b->batch);
    for (int k = 0; k < n; ++k)
        rows[shared ? 0 : members[k]].push_back(Record{(uint32_t)(cells_ij[2 * k + 1] * dim_x + cells_ij[2 * k]), vel_xy[2 * k], vel_xy[2 * k + 1]});
    for (std::vector<Record> &row : rows) unique_by_cell(row);
    // the codes as they stand, for the cells that are fluid now
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(b->stream));   // launches in flight may still read the table this call replaces
    const size_t stride = o.codes_per_member ? b->cells : 0;
    std::vector<uint16_t> codes(o.codes_per_member ? (size_t)b->batch * b->cells : b->cells);
    HIP_TRY(hipMemcpy(codes.data(), o.d_codes, codes.size() * sizeof(uint16_t), hipMemcpyDeviceToHost));
    SFL_TRY(stage_table(b, rows, shared, codes.data(), stride, call));
    o.profile.swap(rows);
    o.profile_shared = shared;
    o.profile_on = true;
    o.profile_step = profile_step;
    o.profile_restage = profile_restage;
    return SFL_OK;
}

int sfl_batch_inflow_profile_info(sfl_batch *b, int *set, int64_t *records)
{
    if (!b) return fail(SFL_ERR_INVALID, "sfl_batch_inflow_profile_info: batch is NULL");
    const sfl_batch::Openings &o = b->openings;
    const bool on = o.set && o.profile_on;
    int64_t held = 0;
    if (on)
        for (const std::vector<Record> &row : o.profile) held += (int64_t)row.size() * (o.profile_shared ? b->batch : 1);
    if (set) *set = on ? 1 : 0;
    if (records) *records = held;
    return SFL_OK;
}

int sfl_batch_inflow_profile_download(sfl_batch *b, int member, int *cells_ij, float *vel_xy, int capacity, int *records)
{
    const char *call = "sfl_batch_inflow_profile_download";
    if (!b) return fail(SFL_ERR_INVALID, "%s: batch is NULL", call);
    if (member < 0 || member >= b->batch) return fail(SFL_ERR_INVALID, "%s: member %d is not inside the batch's [0, %d)", call, member, b->batch);
    if (capacity < 0) return fail(SFL_ERR_INVALID, "%s: capacity must be >= 0 (got %d)", call, capacity);
    const sfl_batch::Openings &o = b->openings;
    static const std::vector<Record> none;
    const std::vector<Record> &row = (o.set && o.profile_on) ? o.profile[o.profile_shared ? 0 : member] : none;
    if (records) *records = (int)row.size();
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

int sfl_batch_openings_flux(sfl_batch *b, int first, int count, struct sfl_open_flux *host, size_t bytes)
{
    const char *call = "sfl_batch_openings_flux";
    if (!b) return fail(SFL_ERR_INVALID, "%s: batch is NULL", call);
    if (first < 0 || count < 0 || (int64_t)first + count > b->batch)
        return fail(SFL_ERR_INVALID, "%s: members [%d, %d + %d) are not inside the batch's [0, %d)", call, first, first, count, b->batch);
    const size_t want = (size_t)count * sizeof(struct sfl_open_flux);
    if (bytes != want) return fail(SFL_ERR_INVALID, "%s: the flux records of %d members are %zu bytes, got %zu", call, count, want, bytes);
    if (count == 0) return SFL_OK;
    if (!host) return fail(SFL_ERR_INVALID, "%s: host is NULL", call);
    sfl_batch::Openings &o = b->openings;
    if (!o.set || o.inflow_cells + o.outflow_cells == 0) {   // nothing live: zeros, no launch
        memset(host, 0, bytes);
        return SFL_OK;
    }
    HIP_TRY(hipSetDevice(b->device));
    if (!o.d_flux) {
        const hipError_t e = hipMalloc(&o.d_flux, (size_t)b->batch * sizeof(struct sfl_open_flux));
        if (e != hipSuccess) {
            (void)hipGetLastError();
            o.d_flux = nullptr;
            return fail(e == hipErrorOutOfMemory ? SFL_ERR_NOMEM : SFL_ERR_HIP, "%s: hipMalloc of the flux records failed: %s", call, hipGetErrorString(e));
        }
    }
    struct sfl_open_flux *d = static_cast<struct sfl_open_flux *>(o.d_flux);
    HIP_TRY(sfl::launch_batch_open_flux(b->stream, d, b->vel, openings_of(b), b->dim_x, b->dim_y, first, count));
    HIP_TRY(hipMemcpyAsync(host, d, bytes, hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return SFL_OK;
}

}  // extern "C"
