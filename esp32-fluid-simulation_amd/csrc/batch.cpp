// batch.cpp -- batches of the C ABI (include/sfl.h group 4, sfl_batch_*): B independent whole-domain simulations of one
// small grid on one device, stepped by ONE launch of B workgroups (batch_grid.hip; batch_large.hip for the batches of
// sfl_batch_create_large -- the only difference on this side is which of the two families of six launchers a call takes).
// Argument checks, field I/O, the staging of queued forces into per-member order, of per-member parameters into device
// records, and the ping-pong of velocity and dye.  Host C++ only; it shares the error plumbing of context.h and nothing
// else with the context units.  batch_state.h has the struct; batch_frames.cpp the frames of many members and the recorder.
#include "batch_state.h"

#include <cmath>

using sfl::host::fail;

namespace {

void release(sfl_batch *b)
{
    (void)hipSetDevice(b->device);
    if (b->stream) (void)hipStreamSynchronize(b->stream);
    for (void *m : {(void *)b->vel, (void *)b->vel_tmp, (void *)b->col, (void *)b->col_tmp, (void *)b->div, (void *)b->p,
                    b->d_forces, (void *)b->d_members, (void *)b->d_report, (void *)b->d_counts, (void *)b->d_image,
                    (void *)b->d_stats, (void *)b->d_images, (void *)b->d_frames, (void *)b->d_dist, (void *)b->d_env,
                    (void *)b->tracers.d_xy, (void *)b->tracers.d_trail, (void *)b->views.d_palette, b->views.d_out,
                    (void *)b->d_rec_palette, b->history.d_records, (void *)b->solids.d_codes,
                    (void *)b->loads.d_labels, b->loads.d_records, b->friction.d_records, b->torque.d_records, (void *)b->torque.d_pivot2, b->means.d_planes, b->viscosity.d_table, (void *)b->openings.d_codes,
                    (void *)b->openings.d_inflow, b->openings.d_profile, b->openings.d_flux, b->walls.d_table})
        if (m) (void)hipFree(m);
    if (b->h_stats) (void)hipHostFree(b->h_stats);
    if (b->h_dist) (void)hipHostFree(b->h_dist);
    for (sfl_batch::Stage *pair : {b->stage, b->member_stage, b->viscosity.stage_slot})
        for (int k = 0; k < 2; ++k) {
            if (pair[k].host) (void)hipHostFree(pair[k].host);
            if (pair[k].copied) (void)hipEventDestroy(pair[k].copied);
        }
    if (b->stream) (void)hipStreamDestroy(b->stream);
    delete b;
}

struct Release {
    void operator()(sfl_batch *b) const { release(b); }
};

size_t elem_bytes(int field)
{
    switch (field) {
        case SFL_FIELD_VELOCITY: return 8;
        case SFL_FIELD_COLOR: return 12;
        case SFL_FIELD_DIVERGENCE:
        case SFL_FIELD_PRESSURE: return 4;
    }
    return 0;
}

void *field_base(sfl_batch *b, int field)
{
    switch (field) {
        case SFL_FIELD_VELOCITY: return b->vel;
        case SFL_FIELD_COLOR: return b->col;
        case SFL_FIELD_DIVERGENCE: return b->div;
        case SFL_FIELD_PRESSURE: return b->p;
    }
    return nullptr;
}

int use_device(sfl_batch *b)
{
    HIP_TRY(hipSetDevice(b->device));
    return SFL_OK;
}

int alloc_field(sfl_batch *b, void **ptr, size_t elem, bool zero)
{
    const size_t bytes = (size_t)b->batch * b->cells * elem;
    HIP_TRY(hipMalloc(ptr, bytes));
    if (zero) HIP_TRY(hipMemsetAsync(*ptr, 0, bytes, b->stream));
    return SFL_OK;
}

// the checks of upload / download: members [first, first + count) of a field, `bytes` of host memory
int check_range(sfl_batch *b, int field, int first, int count, const void *host, size_t bytes)
{
    if (!b) return fail(SFL_ERR_INVALID, "batch is NULL");
    const size_t elem = elem_bytes(field);
    if (!elem) return fail(SFL_ERR_INVALID, "unknown field id %d", field);
    if (first < 0 || count < 0 || (int64_t)first + count > b->batch)
        return fail(SFL_ERR_INVALID, "members [%d, %d + %d) are not inside the batch's [0, %d)", first, first, count, b->batch);
    const size_t want = (size_t)count * b->cells * elem;
    if (bytes != want)
        return fail(SFL_ERR_INVALID, "%d members of field %d are %zu bytes, got %zu", count, field, want, bytes);
    if (!host && count > 0) return fail(SFL_ERR_INVALID, "host is NULL");
    return SFL_OK;
}

// The last step of the timeline that has a record, plus one: 0 for an empty timeline.
int64_t timeline_steps(const sfl_batch *b) { return std::max<int64_t>(b->force_last - b->force_base + 1, 0); }

// The timeline as one CSR table on the device (batch_state.h has the layout), for a call of n steps: a stable counting
// sort by (step, member), so each member keeps its queue order within a step (the last write to a cell wins,
// ino:264-269), copied behind the launches queued so far.  Nothing is done while the table on the device still holds
// the rows this call needs: the timeline is staged once per change, not once per step.  A timeline longer than the call
// is staged beyond it, as far as a table of 2^20 rows x members goes; a later call stages the rest.
int stage_timeline(sfl_batch *b, int n)
{
    const int64_t steps = timeline_steps(b), need = std::min<int64_t>(n, steps);
    if (need == 0) return SFL_OK;
    if (b->forces_staged && b->staged_base <= b->force_base && b->force_base + need <= b->staged_base + b->staged_rows) return SFL_OK;
    const int64_t rows = std::min(steps, std::max<int64_t>(need, (1 << 20) / b->batch));
    size_t n_rec = 0;
    for (const sfl_batch::Force &f : b->forces) n_rec += f.step - b->force_base < rows;
    const size_t n_off = (size_t)rows * b->batch + 1;
    const size_t bytes = sizeof(int) * (n_off + 2 * n_rec) + sizeof(float) * 2 * n_rec;
    sfl_batch::Stage &st = b->stage[b->slot];
    b->slot ^= 1;
    if (!st.copied) HIP_TRY(hipEventCreateWithFlags(&st.copied, hipEventDisableTiming));
    if (st.pending) {
        HIP_TRY(hipEventSynchronize(st.copied));
        st.pending = false;
    }
    if (bytes > st.bytes) {
        if (st.host) (void)hipHostFree(st.host);
        st.host = nullptr;
        st.bytes = 0;
        HIP_TRY(hipHostMalloc(&st.host, bytes, hipHostMallocDefault));
        st.bytes = bytes;
    }
    b->forces_staged = false;
    if (bytes > b->d_forces_bytes) {
        HIP_TRY(hipStreamSynchronize(b->stream));   // an earlier step may still read the old buffer: drain on growth only
        if (b->d_forces) (void)hipFree(b->d_forces);
        b->d_forces = nullptr;
        b->d_forces_bytes = 0;
        HIP_TRY(hipMalloc(&b->d_forces, bytes));
        b->d_forces_bytes = bytes;
    }
    int *off = static_cast<int *>(st.host);
    int *hc = off + n_off;
    float *hv = reinterpret_cast<float *>(hc + 2 * n_rec);
    std::fill(off, off + n_off, 0);
    const auto row_of = [&](const sfl_batch::Force &f) { return (size_t)(f.step - b->force_base) * b->batch + f.member; };
    for (const sfl_batch::Force &f : b->forces)
        if (f.step - b->force_base < rows) ++off[row_of(f) + 1];
    for (size_t m = 1; m < n_off; ++m) off[m] += off[m - 1];
    b->staged_row_has.assign((size_t)rows, 0);
    for (int64_t r = 0; r < rows; ++r) b->staged_row_has[r] = off[(r + 1) * b->batch] > off[r * b->batch];
    std::vector<int> next(off, off + n_off - 1);
    for (const sfl_batch::Force &f : b->forces) {
        if (f.step - b->force_base >= rows) continue;
        const int at = next[row_of(f)]++;
        hc[2 * at] = f.i;
        hc[2 * at + 1] = f.j;
        hv[2 * at] = f.vx;
        hv[2 * at + 1] = f.vy;
    }
    HIP_TRY(hipMemcpyAsync(b->d_forces, st.host, bytes, hipMemcpyHostToDevice, b->stream));
    HIP_TRY(hipEventRecord(st.copied, b->stream));
    st.pending = true;
    b->staged_base = b->force_base;
    b->staged_rows = (int)rows;
    b->staged_records = n_rec;
    b->forces_staged = true;
    return SFL_OK;
}

// The rows of the staged table from step k of the call on (stage_timeline has run): *rows of them, 0 and nullptr when
// the table ends before that step.  cells and vel: the table's records, which a row's offsets index.
const int *staged_rows_from(const sfl_batch *b, int k, int *rows, const int **cells, const float **vel)
{
    const int64_t r = b->force_base + k - b->staged_base;
    *rows = 0;
    *cells = nullptr;
    *vel = nullptr;
    if (!b->forces_staged || r < 0 || r >= b->staged_rows) return nullptr;
    const int *d_off = static_cast<const int *>(b->d_forces);
    const size_t n_off = (size_t)b->staged_rows * b->batch + 1;
    *rows = (int)(b->staged_rows - r);
    *cells = d_off + n_off;
    *vel = reinterpret_cast<const float *>(d_off + n_off + 2 * b->staged_records);
    return d_off + (size_t)r * b->batch;
}

// does any of the steps [first, last) of the call have a record?  (stage_timeline has run: the table holds every row of
// the call that has one)
bool staged_has(const sfl_batch *b, int first, int last)
{
    if (!b->forces_staged) return false;
    for (int64_t r = b->force_base + first - b->staged_base; r < b->force_base + last - b->staged_base && r < b->staged_rows; ++r)
        if (r >= 0 && b->staged_row_has[(size_t)r]) return true;
    return false;
}

// BatchStep::force_offsets of step k of the call: that step's row, nullptr for a step without records (as a call without
// queued forces has always passed)
void step_forces(const sfl_batch *b, int k, sfl::BatchStep *a)
{
    int rows = 0;
    a->force_offsets = staged_rows_from(b, k, &rows, &a->step.force_cells, &a->step.force_vel);
    if (a->force_offsets && !b->staged_row_has[(size_t)(b->force_base + k - b->staged_base)]) a->force_offsets = nullptr;
}

// n steps have been launched: their records go, the later ones move down by n
void consume_forces(sfl_batch *b, int n)
{
    b->force_base += n;
    const auto gone = [&](const sfl_batch::Force &f) { return f.step < b->force_base; };
    b->forces.erase(std::remove_if(b->forces.begin(), b->forces.end(), gone), b->forces.end());
    if (b->forces.empty()) b->force_last = -1;
}

// How a step call runs its solve: the same for every member, per member (and the update norm), per member by the
// stopping rule (and the norm and the iterations).
enum StepKind { kUniform, kEach, kUntil };

// The n steps of a step call, behind its checks and the staging of its members: the timeline staged, the launches, the
// ping-pong, the recorder, the timeline consumed.  `a`: the shape, div, p and, for kUniform, the parameters.
// One launch per step -- but `steps` steps per launch (batch_play.hip) for a call that could not be made before there
// was a timeline: n >= 2 steps of small members with a record in some step of [1, n), not by the stopping rule.  With a
// recorder on, such a call is cut into launches that end at the steps whose frame is due, the render between them.
// With a following set of tracers (tracers_follow) every step is a launch of its own, the advance behind it: the tracers
// read each step's projected velocity, which the launch of several steps never stores.  A history (history_step) cuts
// the call as the recorder does: its sample reads the fields of the step it is due after, and so do the averages (mean_step).  With solid cells set
// (b->solids; solids.cpp) every step is a launch of its own too, made through the batch's pointer, and so it is with a
// viscosity set (b->viscosity; viscous.cpp), whose pointer picks the kernel with or without solids itself.
int run_steps(sfl_batch *b, int n, StepKind kind, sfl::BatchStep a)
{
    SFL_TRY(stage_timeline(b, n));
    if (kind != kUntil && !b->large && n >= 2 && !b->tracers_follow && !b->solids.set && !b->viscosity.set && !b->openings.set && staged_has(b, 1, n)) {
        for (int done = 0; done < n;) {
            const int steps = sfl::host::mean_run(b->means, sfl::host::history_run(b->history, sfl::host::record_run(b, n - done)));   // (cut at any's due steps)
            sfl::BatchPlay play{};
            play.step = a.step;
            play.force_rows = staged_rows_from(b, done, &play.rows, &play.step.force_cells, &play.step.force_vel);
            play.rows = std::min(play.rows, steps);
            play.steps = steps;
            play.step.v_in = b->vel;
            play.step.v_out = b->vel_tmp;
            play.step.col_in = b->col;
            play.step.col_out = b->col_tmp;
            HIP_TRY(sfl::launch_batch_play(b->stream, play, b->batch, kind == kEach ? b->d_members : nullptr, b->d_report));
            std::swap(b->vel, b->vel_tmp);
            if (steps & 1) std::swap(b->col, b->col_tmp);   // (the dye ping-pongs inside the launch)
            SFL_TRY(sfl::host::record_step(b, steps));
            if (b->history_step) SFL_TRY(b->history_step(b, steps, kind == kEach ? b->d_members : nullptr, false, a.step));
            if (b->loads_step) SFL_TRY(b->loads_step(b, steps));   // (no solids here: the samples inside are zeros, no cut)
            if (b->friction_step) SFL_TRY(b->friction_step(b, steps));   // (the same)
            if (b->torque_step) SFL_TRY(b->torque_step(b, steps));       // (the same)
            if (b->mean_step) SFL_TRY(b->mean_step(b, steps));   // (the averages read the fields: mean_run has cut at their due steps)
            done += steps;
        }
        consume_forces(b, n);
        return SFL_OK;
    }
    for (int k = 0; k < n; ++k) {
        step_forces(b, k, &a);
        a.step.v_in = b->vel;
        a.step.v_out = b->vel_tmp;
        a.step.col_in = b->col;
        a.step.col_out = b->col_tmp;
        if (b->walls.step)   // (a wall table is held: never without solids, so never kUntil, never large; walls.cpp picks the kernel)
            SFL_TRY(b->walls.step(b, kind == kEach, a));
        else if (b->viscosity.set)   // (never kUntil, never large: refused at the call and at sfl_batch_set_viscosity)
            SFL_TRY(b->viscosity.step(b, kind == kEach, a));
        else if (b->openings.set)   // (never kUntil, never large, never with viscosity: refused at the calls; its codes hold the solids')
            SFL_TRY(b->openings.step(b, kind == kEach, a));
        else if (b->solids.set)   // (never kUntil, never large: refused at the call and at sfl_batch_set_solids)
            SFL_TRY(b->solids.step(b, kind == kEach, a));
        else if (kind == kUniform)
            HIP_TRY((b->large ? sfl::launch_batch_large_step : sfl::launch_batch_step)(b->stream, a, b->batch));
        else if (kind == kEach)
            HIP_TRY((b->large ? sfl::launch_batch_large_step_each : sfl::launch_batch_step_each)(b->stream, a, b->batch, b->d_members, b->d_report));
        else   // (the first step starts every member's sum of iterations, the later ones add to it)
            HIP_TRY((b->large ? sfl::launch_batch_large_step_until : sfl::launch_batch_step_until)(b->stream, a, b->batch, b->d_members, b->d_stops,
                                                                                               b->d_report, b->d_counts, k > 0));
        std::swap(b->vel, b->vel_tmp);  // ino:255
        std::swap(b->col, b->col_tmp);  // ino:286
        SFL_TRY(sfl::host::record_step(b));
        if (b->tracers_follow) SFL_TRY(b->tracers_follow(b, kind == kUniform ? nullptr : b->d_members, a.step.dt));
        if (b->history_step) SFL_TRY(b->history_step(b, 1, kind == kUniform ? nullptr : b->d_members, kind == kUntil, a.step));
        if (b->loads_step) SFL_TRY(b->loads_step(b, 1));
        if (b->friction_step) SFL_TRY(b->friction_step(b, 1));
        if (b->torque_step) SFL_TRY(b->torque_step(b, 1));
        if (b->mean_step) SFL_TRY(b->mean_step(b, 1));
    }
    consume_forces(b, n);
    return SFL_OK;
}

sfl::SorParams sor_params(float dx, float omega)
{
    sfl::SorParams prm{};
    prm.dx = dx;
    prm.omega = omega;
    prm.one_minus_omega = 1.0f - omega;  // (1 - omega) in float, poisson.cpp:98,111
    prm.neg_quarter_omega = -0.25f * omega;
    prm.fold = 0;                        // (the one-workgroup kernels always multiply twice)
    return prm;
}

// 1 / (2 dx) as the divergence and the gradient use it (finitediff.cpp:36, :78-79)
float two_dx_inv(float dx) { return 1.0f / (2.0f * dx); }

// the checks of the *_each calls on their records: nothing is launched or dequeued before they pass
int check_members(sfl_batch *b, const sfl_member_params *params)
{
    if (!b) return fail(SFL_ERR_INVALID, "batch is NULL");
    if (!params) return fail(SFL_ERR_INVALID, "params is NULL");
    for (int m = 0; m < b->batch; ++m)
        if (params[m].iters < 0)
            return fail(SFL_ERR_INVALID, "member %d: iters must be >= 0 (got %d)", m, (int)params[m].iters);
    return SFL_OK;
}

// ... and of the *_until calls on both kinds of record: the first member with anything wrong is the one named
int check_members(sfl_batch *b, const sfl_member_params *params, const sfl_member_stop *stops)
{
    if (!b) return fail(SFL_ERR_INVALID, "batch is NULL");
    if (!params) return fail(SFL_ERR_INVALID, "params is NULL");
    if (!stops) return fail(SFL_ERR_INVALID, "stops is NULL");
    for (int m = 0; m < b->batch; ++m) {
        if (params[m].iters < 0)
            return fail(SFL_ERR_INVALID, "member %d: iters (the cap) must be >= 0 (got %d)", m, (int)params[m].iters);
        if (stops[m].every < 1)
            return fail(SFL_ERR_INVALID, "member %d: every must be >= 1 (got %d)", m, (int)stops[m].every);
        if (std::isnan(stops[m].tol))
            return fail(SFL_ERR_INVALID, "member %d: tol is a NaN (a negative tol never stops a member, +inf stops it at once)", m);
    }
    return SFL_OK;
}

// The members' records, with the host-derived constants formed as the uniform path forms them, copied to the device
// behind the launches queued so far.  Launch order: when the iteration counts differ, the members with the most go first
// (a stable sort, so the order is a function of the parameters alone) -- workgroups start roughly in that order and a
// long member that starts last would set the launch's end alone; results do not depend on it.  The device array has its
// final size from the first call on and is written in stream order, so nothing ever drains the stream; a pinned slot is
// rewritten only after its last copy has completed.  With `stops` (the *_until calls) the members' stopping rules travel
// behind the records -- same order, same copy, the tail of the same device array (d_stops).
int stage_members(sfl_batch *b, const sfl_member_params *params, const sfl_member_stop *stops = nullptr)
{
    const size_t rec_bytes = sizeof(sfl::BatchMember) * (size_t)b->batch;
    const size_t all_bytes = rec_bytes + sizeof(sfl::BatchStop) * (size_t)b->batch;
    const size_t bytes = stops ? all_bytes : rec_bytes;
    sfl_batch::Stage &st = b->member_stage[b->member_slot];
    b->member_slot ^= 1;
    if (!st.copied) HIP_TRY(hipEventCreateWithFlags(&st.copied, hipEventDisableTiming));
    if (st.pending) {
        HIP_TRY(hipEventSynchronize(st.copied));
        st.pending = false;
    }
    if (!st.host) {
        HIP_TRY(hipHostMalloc(&st.host, all_bytes, hipHostMallocDefault));
        st.bytes = all_bytes;
    }
    if (!b->d_members) {
        HIP_TRY(hipMalloc((void **)&b->d_members, all_bytes));
        b->d_stops = reinterpret_cast<sfl::BatchStop *>(b->d_members + b->batch);
    }
    if (!b->d_report) HIP_TRY(hipMalloc((void **)&b->d_report, sizeof(float) * (size_t)b->batch));
    if (!b->d_counts) HIP_TRY(hipMalloc((void **)&b->d_counts, sizeof(int) * 2 * (size_t)b->batch));
    std::vector<int> order((size_t)b->batch);
    for (int m = 0; m < b->batch; ++m) order[m] = m;
    const auto differs = [&](const sfl_member_params &q) { return q.iters != params[0].iters; };
    if (std::any_of(params, params + b->batch, differs))
        std::stable_sort(order.begin(), order.end(), [&](int l, int r) { return params[l].iters > params[r].iters; });
    sfl::BatchMember *rec = static_cast<sfl::BatchMember *>(st.host);
    for (int k = 0; k < b->batch; ++k) {
        const sfl_member_params &q = params[order[k]];
        rec[k].dt = q.dt;
        rec[k].two_dx_inv = two_dx_inv(q.dx);
        rec[k].prm = sor_params(q.dx, q.omega);
        rec[k].iters = q.iters;
        rec[k].member = order[k];
    }
    if (stops) {
        sfl::BatchStop *stop = reinterpret_cast<sfl::BatchStop *>(rec + b->batch);
        for (int k = 0; k < b->batch; ++k) stop[k] = sfl::BatchStop{stops[order[k]].tol, stops[order[k]].every};
    }
    HIP_TRY(hipMemcpyAsync(b->d_members, st.host, bytes, hipMemcpyHostToDevice, b->stream));
    HIP_TRY(hipEventRecord(st.copied, b->stream));
    st.pending = true;
    return SFL_OK;
}

// sfl_batch_flow_stats and its _each form: dx for every member, or params[m].dx (each).  The checks that need no batch come
// first, so that each of them answers with its own message on a box without a GPU too.
int flow_stats(sfl_batch *b, int what, float dx, bool each, const sfl_member_params *params, int first, int count,
               struct sfl_flow_stats *host, size_t bytes)
{
    if (what == 0 || (what & ~(SFL_STATS_VELOCITY | SFL_STATS_DYE)))
        return fail(SFL_ERR_INVALID, "what must be SFL_STATS_VELOCITY (1), SFL_STATS_DYE (2) or both (got %d)", what);
    if (count < 0 || bytes != (size_t)count * sizeof(struct sfl_flow_stats))
        return fail(SFL_ERR_INVALID, "the flow statistics of %d members are %zu bytes, got %zu", count,
                    (size_t)std::max(count, 0) * sizeof(struct sfl_flow_stats), bytes);
    if (!b || !host || (each && !params)) return fail(SFL_ERR_INVALID, "NULL argument");
    if (first < 0 || (int64_t)first + count > b->batch)
        return fail(SFL_ERR_INVALID, "members [%d, %d + %d) are not inside the batch's [0, %d)", first, first, count, b->batch);
    if (count == 0) return SFL_OK;
    SFL_TRY(use_device(b));
    const size_t rec_bytes = sizeof(sfl::FlowStatsRecord) * (size_t)b->batch, all_bytes = rec_bytes + sizeof(float) * (size_t)b->batch;
    if (!b->d_stats) HIP_TRY(hipMalloc((void **)&b->d_stats, all_bytes));
    if (!b->h_stats) HIP_TRY(hipHostMalloc((void **)&b->h_stats, all_bytes, hipHostMallocDefault));
    // (the call is synchronous: the pinned block is never in flight when the next call writes it)
    const float *d_scale = nullptr;
    if (each && (what & SFL_STATS_VELOCITY)) {
        float *scale = reinterpret_cast<float *>(b->h_stats + b->batch);
        for (int m = 0; m < b->batch; ++m) scale[m] = two_dx_inv(params[m].dx);
        HIP_TRY(hipMemcpyAsync(b->d_stats + b->batch, scale, sizeof(float) * (size_t)b->batch, hipMemcpyHostToDevice, b->stream));
        d_scale = reinterpret_cast<const float *>(b->d_stats + b->batch);
    }
    if ((b->solids.set || b->openings.set) && (what & SFL_STATS_VELOCITY)) {   // the records zeroed and the dye pass as ever, the velocity pass by the solids' or the openings' rule
        HIP_TRY(sfl::launch_flow_stats(b->stream, b->d_stats, what & SFL_STATS_DYE, b->vel, b->col, b->dim_x, b->dim_y, b->batch, two_dx_inv(dx), d_scale));
        SFL_TRY((b->openings.set ? b->openings.stats : b->solids.stats)(b, two_dx_inv(dx), d_scale));
    } else
        HIP_TRY(sfl::launch_flow_stats(b->stream, b->d_stats, what, b->vel, b->col, b->dim_x, b->dim_y, b->batch, two_dx_inv(dx), d_scale));
    HIP_TRY(hipMemcpyAsync(b->h_stats + first, b->d_stats + first, (size_t)count * sizeof(struct sfl_flow_stats), hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    memcpy(host, b->h_stats + first, (size_t)count * sizeof(struct sfl_flow_stats));
    for (int k = 0; k < count; ++k) host[k].what = (uint32_t)what;
    return SFL_OK;
}

// the *_until calls of a batch with solid cells: refused whole (include/sfl.h "SOLIDS"), nothing staged or launched
int refuse_until(const char *call)
{
    return fail(SFL_ERR_STATE, "%s: the batch has solid cells set (sfl_batch_set_solids) and the solve to a tolerance does not know them: "
                "nothing stepped or solved; use the _each call, or clear the solids with sfl_batch_set_solids(b, NULL, 0)", call);
}

// ... and of a batch with openings (include/sfl.h "OPENINGS")
int refuse_until_open(const char *call)
{
    return fail(SFL_ERR_STATE, "%s: the batch has openings set (sfl_batch_set_openings) and the solve to a tolerance does not know them: "
                "nothing stepped or solved; use the _each call, or clear the openings with sfl_batch_set_openings(b, NULL, 0, NULL, 0)", call);
}

// what both constructors do once their limits have passed: the device, the stream, the six zeroed fields
int make_batch(sfl_batch **out, int device, int dim_x, int dim_y, int batch, bool large)
{
    int ndev = 0;
    SFL_TRY(sfl_device_count(&ndev));
    if (device < 0 || device >= ndev) return fail(SFL_ERR_HIP, "device %d not available (%d visible)", device, ndev);

    std::unique_ptr<sfl_batch, Release> b(new sfl_batch);
    b->device = device;
    b->dim_x = dim_x;
    b->dim_y = dim_y;
    b->batch = batch;
    b->cells = (size_t)dim_x * (size_t)dim_y;
    b->large = large;
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking));
    SFL_TRY(alloc_field(b.get(), (void **)&b->vel, 8, true));
    SFL_TRY(alloc_field(b.get(), (void **)&b->vel_tmp, 8, false));
    SFL_TRY(alloc_field(b.get(), (void **)&b->col, 12, true));
    SFL_TRY(alloc_field(b.get(), (void **)&b->col_tmp, 12, false));
    SFL_TRY(alloc_field(b.get(), (void **)&b->div, 4, true));
    SFL_TRY(alloc_field(b.get(), (void **)&b->p, 4, true));
    HIP_TRY(hipStreamSynchronize(b->stream));
    *out = b.release();
    return SFL_OK;
}

}  // namespace

extern "C" {

int sfl_batch_create(sfl_batch **out, int device, int dim_x, int dim_y, int batch)
{
    if (!out) return fail(SFL_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (dim_x < 2 || dim_y < 2) return fail(SFL_ERR_INVALID, "dim_x and dim_y must be >= 2 (got %d x %d)", dim_x, dim_y);
    if (batch < 1) return fail(SFL_ERR_INVALID, "batch must be >= 1 (got %d)", batch);
    const int64_t cells = (int64_t)dim_x * dim_y;
    if (cells > sfl::kSmallGridMaxCells)
        return fail(SFL_ERR_INVALID, "a batch member holds at most %d cells (one workgroup's LDS): %d x %d has %lld",
                    sfl::kSmallGridMaxCells, dim_x, dim_y, (long long)cells);
    if (!sfl::small_grid_fits(dim_x, dim_y))
        return fail(SFL_ERR_INVALID, "a batch member holds at most %d cells of one colour (dim_y * ceil(dim_x / 2), the "
                    "cells one workgroup's threads own): %d x %d has %lld", sfl::kSmallGridMaxCells / 2, dim_x, dim_y,
                    (long long)dim_y * ((dim_x + 1) / 2));
    if ((int64_t)batch * cells > INT32_MAX)
        return fail(SFL_ERR_INVALID, "batch x cells must be <= 2^31 - 1 (got %d x %lld)", batch, (long long)cells);
    return make_batch(out, device, dim_x, dim_y, batch, false);
}

int sfl_batch_create_large(sfl_batch **out, int device, int dim_x, int dim_y, int batch)
{
    static_assert(SFL_BATCH_LARGE_MAX_CELLS == sfl::kLargeMemberMaxCells, "include/sfl.h and batch.h state one limit");
    if (!out) return fail(SFL_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (dim_x < 2 || dim_y < 2) return fail(SFL_ERR_INVALID, "dim_x and dim_y must be >= 2 (got %d x %d)", dim_x, dim_y);
    if (batch < 1) return fail(SFL_ERR_INVALID, "batch must be >= 1 (got %d)", batch);
    const int64_t cells = (int64_t)dim_x * dim_y;
    if (cells > sfl::kLargeMemberMaxCells)
        return fail(SFL_ERR_INVALID, "a large batch member holds at most %d cells (its divergence and pressure in one "
                    "workgroup's LDS): %d x %d has %lld", sfl::kLargeMemberMaxCells, dim_x, dim_y, (long long)cells);
    if (!sfl::large_member_fits(dim_x, dim_y))
        return fail(SFL_ERR_INVALID, "a large batch member holds at most %d cells of one colour (dim_y * ceil(dim_x / 2), the "
                    "cells one workgroup's threads own): %d x %d has %lld", sfl::kLargeMemberMaxColour, dim_x, dim_y,
                    (long long)dim_y * ((dim_x + 1) / 2));
    if ((int64_t)batch * cells > INT32_MAX)
        return fail(SFL_ERR_INVALID, "batch x cells must be <= 2^31 - 1 (got %d x %lld)", batch, (long long)cells);
    return make_batch(out, device, dim_x, dim_y, batch, true);
}

int sfl_batch_is_large(sfl_batch *b, int *large)
{
    if (!b || !large) return fail(SFL_ERR_INVALID, "NULL argument");
    *large = b->large ? 1 : 0;
    return SFL_OK;
}

int sfl_batch_destroy(sfl_batch *b)
{
    if (!b) return fail(SFL_ERR_INVALID, "batch is NULL");
    release(b);
    return SFL_OK;
}

int sfl_batch_shape(sfl_batch *b, int *dim_x, int *dim_y, int *batch)
{
    if (!b) return fail(SFL_ERR_INVALID, "batch is NULL");
    if (dim_x) *dim_x = b->dim_x;
    if (dim_y) *dim_y = b->dim_y;
    if (batch) *batch = b->batch;
    return SFL_OK;
}

int sfl_batch_upload(sfl_batch *b, int field, int first, int count, const void *host, size_t bytes)
{
    SFL_TRY(check_range(b, field, first, count, host, bytes));
    if (count == 0) return SFL_OK;
    SFL_TRY(use_device(b));
    if (field == SFL_FIELD_DIVERGENCE || field == SFL_FIELD_PRESSURE) b->report_valid = b->counts_valid = false;
    char *dev = static_cast<char *>(field_base(b, field)) + (size_t)first * b->cells * elem_bytes(field);
    HIP_TRY(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return SFL_OK;
}

int sfl_batch_download(sfl_batch *b, int field, int first, int count, void *host, size_t bytes)
{
    SFL_TRY(check_range(b, field, first, count, host, bytes));
    if (count == 0) return SFL_OK;
    SFL_TRY(use_device(b));
    const char *dev = static_cast<const char *>(field_base(b, field)) + (size_t)first * b->cells * elem_bytes(field);
    HIP_TRY(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return SFL_OK;
}

int sfl_batch_field_device_ptr(sfl_batch *b, int field, void **dev_ptr)
{
    if (!b || !dev_ptr) return fail(SFL_ERR_INVALID, "NULL argument");
    if (!elem_bytes(field)) return fail(SFL_ERR_INVALID, "unknown field id %d", field);
    *dev_ptr = field_base(b, field);
    return SFL_OK;
}

int sfl_batch_queue_forces_at(sfl_batch *b, int step, const int *members, const int *cells_ij, const float *vel_xy, int n)
{
    if (!b || n < 0 || (n > 0 && (!members || !cells_ij || !vel_xy))) return fail(SFL_ERR_INVALID, "bad arguments");
    if (step < 0) return fail(SFL_ERR_INVALID, "step must be >= 0 (got %d): nothing queued", step);
    for (int k = 0; k < n; ++k)   // all or nothing
        if (members[k] < 0 || members[k] >= b->batch)
            return fail(SFL_ERR_INVALID, "force %d names member %d, outside the batch's [0, %d): nothing queued", k,
                        members[k], b->batch);
    for (int k = 0; k < n; ++k)
        b->forces.push_back({b->force_base + step, members[k], cells_ij[2 * k], cells_ij[2 * k + 1], vel_xy[2 * k], vel_xy[2 * k + 1]});
    if (n > 0) {
        b->forces_staged = false;
        b->force_last = std::max(b->force_last, b->force_base + step);
    }
    return SFL_OK;
}

int sfl_batch_queue_forces(sfl_batch *b, const int *members, const int *cells_ij, const float *vel_xy, int n)
{
    return sfl_batch_queue_forces_at(b, 0, members, cells_ij, vel_xy, n);
}

int sfl_batch_forces_pending(sfl_batch *b, int *records, int *last_step)
{
    if (!b) return fail(SFL_ERR_INVALID, "batch is NULL");
    if (records) *records = (int)std::min<size_t>(b->forces.size(), INT_MAX);
    if (last_step) *last_step = (int)(timeline_steps(b) - 1);
    return SFL_OK;
}

int sfl_batch_forget_forces(sfl_batch *b)
{
    if (!b) return fail(SFL_ERR_INVALID, "batch is NULL");
    b->forces.clear();
    b->forces_staged = false;
    b->force_last = -1;
    return SFL_OK;
}

int sfl_batch_step_n(sfl_batch *b, int n, float dt, float dx, int iters, float omega)
{
    if (!b) return fail(SFL_ERR_INVALID, "batch is NULL");
    if (n < 0) return fail(SFL_ERR_INVALID, "n must be >= 0 (got %d)", n);
    if (iters < 0) return fail(SFL_ERR_INVALID, "iters must be >= 0 (got %d)", iters);
    if (n == 0) return SFL_OK;
    SFL_TRY(sfl::host::record_admit(b, n));   // a recorder without room for this call's frames refuses it whole
    SFL_TRY(sfl::host::trail_admit_steps(b->tracers, n));   // ... and so does a trail of following tracers without room for its slots
    SFL_TRY(sfl::host::history_admit(b->history, n));   // ... and a history without room for its samples
    SFL_TRY(sfl::host::loads_admit(b->loads, n));       // ... and a loads recorder without room for its
    SFL_TRY(sfl::host::friction_admit(b->friction, n)); // ... and a friction recorder without room for its
    SFL_TRY(sfl::host::torque_admit(b->torque, n));     // ... and a torque recorder without room for its
    SFL_TRY(use_device(b));
    b->report_valid = b->counts_valid = false;   // (the uniform kernels leave no update norm)
    sfl::BatchStep a{};
    a.step.div = b->div;
    a.step.p = b->p;
    a.step.dim_x = b->dim_x;
    a.step.dim_y = b->dim_y;
    a.step.iters = iters;
    a.step.dt = dt;
    a.step.two_dx_inv = two_dx_inv(dx);
    a.step.prm = sor_params(dx, omega);
    if (b->viscosity.set) SFL_TRY(b->viscosity.stage(b, dt, dx, nullptr));   // every member's a and c of this call's dt and dx
    SFL_TRY(run_steps(b, n, kUniform, a));
    return SFL_OK;
}

int sfl_batch_poisson_solve(sfl_batch *b, float dx, int iters, float omega)
{
    if (!b) return fail(SFL_ERR_INVALID, "batch is NULL");
    if (iters < 0) return fail(SFL_ERR_INVALID, "iters must be >= 0 (got %d)", iters);
    SFL_TRY(use_device(b));
    b->report_valid = b->counts_valid = false;
    if (b->openings.set) return b->openings.solve(b, false, iters, sor_params(dx, omega));
    if (b->solids.set) return b->solids.solve(b, false, iters, sor_params(dx, omega));
    HIP_TRY((b->large ? sfl::launch_batch_large_solve : sfl::launch_batch_solve)(b->stream, b->p, b->div, b->dim_x, b->dim_y, b->batch,
                                                                                 iters, sor_params(dx, omega)));
    return SFL_OK;
}

int sfl_batch_step_n_each(sfl_batch *b, int n, const sfl_member_params *params)
{
    SFL_TRY(check_members(b, params));
    if (n < 0) return fail(SFL_ERR_INVALID, "n must be >= 0 (got %d)", n);
    if (n == 0) return SFL_OK;
    SFL_TRY(sfl::host::record_admit(b, n));   // a recorder without room for this call's frames refuses it whole
    SFL_TRY(sfl::host::trail_admit_steps(b->tracers, n));   // ... and so does a trail of following tracers without room for its slots
    SFL_TRY(sfl::host::history_admit(b->history, n));   // ... and a history without room for its samples
    SFL_TRY(sfl::host::loads_admit(b->loads, n));       // ... and a loads recorder without room for its
    SFL_TRY(sfl::host::friction_admit(b->friction, n)); // ... and a friction recorder without room for its
    SFL_TRY(sfl::host::torque_admit(b->torque, n));     // ... and a torque recorder without room for its
    SFL_TRY(use_device(b));
    SFL_TRY(stage_members(b, params));
    if (b->viscosity.set) SFL_TRY(b->viscosity.stage(b, 0.0f, 0.0f, params));   // every member's a and c of its own dt and dx
    b->report_valid = b->counts_valid = false;   // until every launch below is queued; no iterations to report afterwards
    sfl::BatchStep a{};   // (dt, two_dx_inv, iters and prm come from the members' records)
    a.step.div = b->div;
    a.step.p = b->p;
    a.step.dim_x = b->dim_x;
    a.step.dim_y = b->dim_y;
    SFL_TRY(run_steps(b, n, kEach, a));
    b->report_valid = true;   // of the last step's solve: the divergence and pressure a download hands out now
    return SFL_OK;
}

int sfl_batch_poisson_solve_each(sfl_batch *b, const sfl_member_params *params)
{
    SFL_TRY(check_members(b, params));
    SFL_TRY(use_device(b));
    SFL_TRY(stage_members(b, params));
    b->report_valid = b->counts_valid = false;
    if (b->openings.set)
        SFL_TRY(b->openings.solve(b, true, 0, sfl::SorParams{}));
    else if (b->solids.set)
        SFL_TRY(b->solids.solve(b, true, 0, sfl::SorParams{}));
    else
        HIP_TRY((b->large ? sfl::launch_batch_large_solve_each : sfl::launch_batch_solve_each)(b->stream, b->p, b->div, b->dim_x, b->dim_y,
                                                                                               b->batch, b->d_members, b->d_report));
    b->report_valid = true;
    return SFL_OK;
}

int sfl_batch_step_n_until(sfl_batch *b, int n, const sfl_member_params *params, const sfl_member_stop *stops)
{
    SFL_TRY(check_members(b, params, stops));
    if (n < 0) return fail(SFL_ERR_INVALID, "n must be >= 0 (got %d)", n);
    if (b->solids.set) return refuse_until("sfl_batch_step_n_until");
    if (b->openings.set) return refuse_until_open("sfl_batch_step_n_until");
    if (b->viscosity.set)
        return fail(SFL_ERR_STATE, "sfl_batch_step_n_until: the batch has a viscosity set (sfl_batch_set_viscosity) and the step to a tolerance does not "
                    "know it: nothing stepped; use sfl_batch_step_n_each, or clear the viscosity with sfl_batch_set_viscosity(b, NULL, 0, 0)");
    if (n == 0) return SFL_OK;
    SFL_TRY(sfl::host::record_admit(b, n));   // a recorder without room for this call's frames refuses it whole
    SFL_TRY(sfl::host::trail_admit_steps(b->tracers, n));   // ... and so does a trail of following tracers without room for its slots
    SFL_TRY(sfl::host::history_admit(b->history, n));   // ... and a history without room for its samples
    SFL_TRY(sfl::host::loads_admit(b->loads, n));       // ... and a loads recorder without room for its
    SFL_TRY(sfl::host::friction_admit(b->friction, n)); // ... and a friction recorder without room for its
    SFL_TRY(sfl::host::torque_admit(b->torque, n));     // ... and a torque recorder without room for its
    SFL_TRY(use_device(b));
    SFL_TRY(stage_members(b, params, stops));
    b->report_valid = b->counts_valid = false;   // until every launch below is queued
    sfl::BatchStep a{};   // (dt, two_dx_inv, iters and prm come from the members' records)
    a.step.div = b->div;
    a.step.p = b->p;
    a.step.dim_x = b->dim_x;
    a.step.dim_y = b->dim_y;
    SFL_TRY(run_steps(b, n, kUntil, a));
    b->report_valid = b->counts_valid = true;   // of the last step's solve; the sum over all n
    return SFL_OK;
}

int sfl_batch_poisson_solve_until(sfl_batch *b, const sfl_member_params *params, const sfl_member_stop *stops)
{
    SFL_TRY(check_members(b, params, stops));
    if (b->solids.set) return refuse_until("sfl_batch_poisson_solve_until");
    if (b->openings.set) return refuse_until_open("sfl_batch_poisson_solve_until");
    SFL_TRY(use_device(b));
    SFL_TRY(stage_members(b, params, stops));
    b->report_valid = b->counts_valid = false;
    HIP_TRY((b->large ? sfl::launch_batch_large_solve_until : sfl::launch_batch_solve_until)(b->stream, b->p, b->div, b->dim_x, b->dim_y, b->batch,
                                                                                             b->d_members, b->d_stops, b->d_report, b->d_counts));
    b->report_valid = b->counts_valid = true;
    return SFL_OK;
}

int sfl_batch_residual(sfl_batch *b, int first, int count, float *host, size_t bytes)
{
    if (!b) return fail(SFL_ERR_INVALID, "batch is NULL");
    if (first < 0 || count < 0 || (int64_t)first + count > b->batch)
        return fail(SFL_ERR_INVALID, "members [%d, %d + %d) are not inside the batch's [0, %d)", first, first, count, b->batch);
    if (bytes != (size_t)count * sizeof(float))
        return fail(SFL_ERR_INVALID, "the update norm of %d members is %zu bytes, got %zu", count, (size_t)count * sizeof(float), bytes);
    if (!host && count > 0) return fail(SFL_ERR_INVALID, "host is NULL");
    if (!b->report_valid)
        return fail(SFL_ERR_STATE, "no update norm to report: the last call that wrote the divergence or the pressure was not "
                    "sfl_batch_step_n_each or sfl_batch_poisson_solve_each (or their _until forms); call one of them first");
    if (count == 0) return SFL_OK;
    SFL_TRY(use_device(b));
    HIP_TRY(hipMemcpyAsync(host, b->d_report + first, bytes, hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return SFL_OK;
}

int sfl_batch_iterations(sfl_batch *b, int first, int count, int32_t *host, size_t bytes)
{
    if (!b) return fail(SFL_ERR_INVALID, "batch is NULL");
    if (first < 0 || count < 0 || (int64_t)first + count > b->batch)
        return fail(SFL_ERR_INVALID, "members [%d, %d + %d) are not inside the batch's [0, %d)", first, first, count, b->batch);
    if (bytes != (size_t)count * 2 * sizeof(int32_t))
        return fail(SFL_ERR_INVALID, "the iterations of %d members are %zu bytes, got %zu", count,
                    (size_t)count * 2 * sizeof(int32_t), bytes);
    if (!host && count > 0) return fail(SFL_ERR_INVALID, "host is NULL");
    if (!b->counts_valid)
        return fail(SFL_ERR_STATE, "no iterations to report: the last call that wrote the divergence or the pressure was not "
                    "sfl_batch_step_n_until or sfl_batch_poisson_solve_until; call one of them first");
    if (count == 0) return SFL_OK;
    SFL_TRY(use_device(b));
    HIP_TRY(hipMemcpyAsync(host, b->d_counts + 2 * (size_t)first, bytes, hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return SFL_OK;
}

int sfl_batch_flow_stats(sfl_batch *b, int what, float dx, int first, int count, struct sfl_flow_stats *host, size_t bytes)
{
    return flow_stats(b, what, dx, false, nullptr, first, count, host, bytes);
}

int sfl_batch_flow_stats_each(sfl_batch *b, int what, const sfl_member_params *params, int first, int count,
                              struct sfl_flow_stats *host, size_t bytes)
{
    return flow_stats(b, what, 1.0f, true, params, first, count, host, bytes);
}

// Member 0 as sfl_setup_sketch_fields makes it, then copied to the others by doubling: 1 -> 2 -> 4 ... members, a
// copy per doubling instead of a setup per member.
int sfl_batch_setup_sketch_fields(sfl_batch *b)
{
    if (!b) return fail(SFL_ERR_INVALID, "batch is NULL");
    SFL_TRY(use_device(b));
    HIP_TRY(sfl::launch_setup_sketch_fields(b->stream, b->vel, b->col, b->dim_x, b->dim_y));
    for (size_t have = 1; have < (size_t)b->batch; have *= 2) {
        const size_t more = std::min(have, (size_t)b->batch - have) * b->cells;
        HIP_TRY(hipMemcpyAsync(b->vel + 2 * have * b->cells, b->vel, more * 8, hipMemcpyDeviceToDevice, b->stream));
        HIP_TRY(hipMemcpyAsync(b->col + 3 * have * b->cells, b->col, more * 12, hipMemcpyDeviceToDevice, b->stream));
    }
    return SFL_OK;
}

int sfl_batch_render_rgb565(sfl_batch *b, int member, int scaling, int byteswap, uint16_t *host_image, size_t bytes)
{
    if (!b || !host_image) return fail(SFL_ERR_INVALID, "NULL argument");
    if (member < 0 || member >= b->batch)
        return fail(SFL_ERR_INVALID, "member %d outside the batch's [0, %d)", member, b->batch);
    if (scaling < 1 || scaling > 64) return fail(SFL_ERR_INVALID, "scaling must be 1..64 (got %d)", scaling);
    const size_t w = (size_t)scaling * (b->dim_y - 1), h = (size_t)scaling * (b->dim_x - 1);
    if (bytes != w * h * 2) return fail(SFL_ERR_INVALID, "image is %zu x %zu uint16 = %zu bytes, got %zu", h, w, w * h * 2, bytes);
    SFL_TRY(use_device(b));
    if (bytes > b->d_image_bytes) {  // the frame buffer stays with the batch between frames
        if (b->d_image) {
            HIP_TRY(hipStreamSynchronize(b->stream));
            (void)hipFree(b->d_image);
            b->d_image = nullptr;
            b->d_image_bytes = 0;
        }
        void *img = nullptr;
        HIP_TRY(hipMalloc(&img, bytes));
        b->d_image = static_cast<uint16_t *>(img);
        b->d_image_bytes = bytes;
    }
    HIP_TRY(sfl::launch_render_rgb565(b->stream, b->d_image, b->col + 3 * (size_t)member * b->cells, b->dim_x, b->dim_y,
                                      scaling, byteswap != 0));
    HIP_TRY(hipMemcpyAsync(host_image, b->d_image, bytes, hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));  // the caller reads host_image on return
    return SFL_OK;
}

int sfl_batch_synchronize(sfl_batch *b)
{
    if (!b) return fail(SFL_ERR_INVALID, "batch is NULL");
    SFL_TRY(use_device(b));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return SFL_OK;
}

}  // extern "C"
