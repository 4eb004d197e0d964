// tracers.cpp -- points that move with the flow (include/sfl.h "TRACERS"; sfl_tracers_* of a whole-domain context,
// sfl_batch_tracers_* of a batch of either kind): the set a context or batch holds, manual advances, samples of one field
// at the tracers, trails, and the advance behind every step of a step call while a set follows.  Host C++ only; the
// kernels are tracers.hip (tracer_kernels.h).
//
// The step calls live in units that the host test harnesses link without this one, so they do not call into it: the set
// is plain data on the two structs (context.h TracerSet; freed by the destroy paths, a trail's room checked by the step
// calls themselves), and the advance is reached through their `tracers_follow` pointer, set here while a following set
// is attached and null otherwise -- then a step call launches exactly what it launched before there were tracers.
//
// One body serves contexts and batches: a Holder names the set, the stream, the shape and the member count (1 for a
// context).  One device allocation per set: the positions, behind them 12 bytes per tracer for the samples of the widest
// field, so that nothing is allocated per call.
#include "batch_state.h"
#include "tracer_kernels.h"

using namespace sfl::host;

namespace {

struct Holder {
    TracerSet *t;
    hipStream_t stream;
    int device, members, dim_x, dim_y;
    size_t cells;   // of one member
};

Holder holder_of(sfl_context *c)
{
    return Holder{&c->tracers, c->stream, c->device, 1, c->dim_x, c->gdim_y, (size_t)c->dim_x * c->gdim_y};
}
Holder holder_of(sfl_batch *b) { return Holder{&b->tracers, b->stream, b->device, b->batch, b->dim_x, b->dim_y, b->cells}; }

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

const void *field_of(sfl_context *c, int field) { return field_ptr(c, field); }
const void *field_of(sfl_batch *b, int field)
{
    switch (field) {
        case SFL_FIELD_VELOCITY: return b->vel;
        case SFL_FIELD_COLOR: return b->col;
        case SFL_FIELD_DIVERGENCE: return b->div;
        case SFL_FIELD_PRESSURE: return b->p;
    }
    return nullptr;
}

// the checks a call makes on its handle before anything else is looked at
int check_handle(sfl_context *c, const char *call)
{
    if (!c) return fail(SFL_ERR_INVALID, "%s: NULL argument", call);
    if (c->nranks != 1)   // (a slab's tracers would have to change ranks with the rows they cross)
        return fail(SFL_ERR_STATE, "%s: whole-domain contexts only (slab %d/%d)", call, c->rank, c->nranks);
    return SFL_OK;
}
int check_handle(sfl_batch *b, const char *call)
{
    if (!b) return fail(SFL_ERR_INVALID, "%s: NULL argument", call);
    return SFL_OK;
}

// the fields a context would hand out at this moment (as sfl_flow_stats settles them); a batch always holds its own
int settle(sfl_context *c, int field)
{
    SFL_TRY(settle_color(c, true));
    SFL_TRY(check_wait_error(c));
    SFL_TRY(ensure_field(c, field));
    return SFL_OK;
}
int settle(sfl_batch *, int) { return SFL_OK; }

size_t all_tracers(const Holder &h) { return (size_t)h.members * h.t->count; }
size_t slot_floats(const Holder &h) { return 2 * all_tracers(h); }
float *sample_scratch(const Holder &h) { return h.t->d_xy + 2 * all_tracers(h); }

sfl::TracerGrid grid_of(const Holder &h)
{
    return sfl::TracerGrid{h.t->d_xy, (unsigned)h.t->count, h.members, h.dim_x, h.dim_y, h.cells};
}

int no_set(const char *call) { return fail(SFL_ERR_STATE, "%s: no tracers attached: call sfl_tracers_set (sfl_batch_tracers_set) first", call); }

// the set and its trail go; launches that still read them are waited for
int drop(const Holder &h)
{
    TracerSet &t = *h.t;
    if (t.d_xy || t.d_trail) {
        HIP_TRY(hipSetDevice(h.device));
        HIP_TRY(hipStreamSynchronize(h.stream));
        if (t.d_xy) (void)hipFree(t.d_xy);
        if (t.d_trail) (void)hipFree(t.d_trail);
    }
    t = TracerSet{};
    return SFL_OK;
}

int set(const Holder &h, const float *xy, size_t n, int follow)
{
    if (n > (size_t)INT_MAX) return fail(SFL_ERR_INVALID, "at most 2^31 - 1 tracers per context or member (got %zu)", n);
    if (n > 0 && !xy) return fail(SFL_ERR_INVALID, "xy is NULL");
    if (n > 0 && (size_t)h.members > SIZE_MAX / (20 * n))
        return fail(SFL_ERR_INVALID, "%zu tracers in each of %d members exceed the address space", n, h.members);
    SFL_TRY(drop(h));
    if (n == 0) return SFL_OK;
    HIP_TRY(hipSetDevice(h.device));
    const size_t all = (size_t)h.members * n;
    void *mem = nullptr;
    HIP_TRY(hipMalloc(&mem, all * 20));   // 8 bytes of position and 12 of sample scratch per tracer
    TracerSet &t = *h.t;
    t.d_xy = static_cast<float *>(mem);
    t.count = n;
    t.follow = follow != 0;
    const int rc = [&] {
        HIP_TRY(hipMemcpyAsync(t.d_xy, xy, all * 8, hipMemcpyHostToDevice, h.stream));
        HIP_TRY(hipStreamSynchronize(h.stream));
        return SFL_OK;
    }();
    if (rc != SFL_OK) (void)drop(h);
    return rc;
}

int download(const Holder &h, float *xy, size_t capacity, const char *call)
{
    if (!xy) return fail(SFL_ERR_INVALID, "%s: NULL argument", call);
    if (h.t->count == 0) return no_set(call);
    if (capacity < slot_floats(h))
        return fail(SFL_ERR_INVALID, "%s: the positions are %zu floats, capacity is %zu", call, slot_floats(h), capacity);
    HIP_TRY(hipSetDevice(h.device));
    HIP_TRY(hipMemcpyAsync(xy, h.t->d_xy, slot_floats(h) * sizeof(float), hipMemcpyDeviceToHost, h.stream));
    HIP_TRY(hipStreamSynchronize(h.stream));
    return SFL_OK;
}

// One advance on `velocity` (member 0's), launched on the holder's stream; counted by the trail, and the one that makes
// the count a multiple of `every` also writes the next slot (trail_admit has let the call through: there is one).
int advance(const Holder &h, const float *velocity, const sfl::BatchMember *records, float dt)
{
    TracerSet &t = *h.t;
    float *slot = nullptr;
    if (t.trail_on && (t.advances + 1) % t.every == 0) slot = t.d_trail + (size_t)t.written * slot_floats(h);
    HIP_TRY(hipSetDevice(h.device));
    HIP_TRY(sfl::launch_tracer_advance(h.stream, grid_of(h), velocity, records, dt, slot));
    if (t.trail_on) ++t.advances;
    if (slot) ++t.written;
    return SFL_OK;
}

int follow_context(sfl_context *c, float dt) { return advance(holder_of(c), c->vel, nullptr, dt); }
int follow_batch(sfl_batch *b, const sfl::BatchMember *records, float dt) { return advance(holder_of(b), b->vel, records, dt); }

template <class H>
int advance_now(H *x, float dt, const char *call)
{
    SFL_TRY(check_handle(x, call));
    const Holder h = holder_of(x);
    if (h.t->count == 0) return no_set(call);
    SFL_TRY(trail_admit(*h.t, 1));
    SFL_TRY(settle(x, SFL_FIELD_VELOCITY));
    return advance(h, static_cast<const float *>(field_of(x, SFL_FIELD_VELOCITY)), nullptr, dt);
}

template <class H>
int sample_now(H *x, int field, int no_slip, void *out, size_t capacity_bytes, const char *call)
{
    const size_t elem = elem_bytes(field);
    if (!elem)
        return fail(SFL_ERR_INVALID, "%s: unknown field id %d: SFL_FIELD_VELOCITY (0), SFL_FIELD_COLOR (1), SFL_FIELD_DIVERGENCE (2) or "
                    "SFL_FIELD_PRESSURE (3)", call, field);
    SFL_TRY(check_handle(x, call));
    if (!out) return fail(SFL_ERR_INVALID, "%s: NULL argument", call);
    const Holder h = holder_of(x);
    if (h.t->count == 0) return no_set(call);
    const size_t bytes = all_tracers(h) * elem;
    if (capacity_bytes < bytes)
        return fail(SFL_ERR_INVALID, "%s: the samples of field %d are %zu bytes, capacity is %zu", call, field, bytes, capacity_bytes);
    SFL_TRY(settle(x, field));
    HIP_TRY(hipSetDevice(h.device));
    // (the call is synchronous: the scratch is never in flight when the next call writes it)
    HIP_TRY(sfl::launch_tracer_sample(h.stream, grid_of(h), field, field_of(x, field), no_slip != 0, sample_scratch(h)));
    HIP_TRY(hipMemcpyAsync(out, sample_scratch(h), bytes, hipMemcpyDeviceToHost, h.stream));
    HIP_TRY(hipStreamSynchronize(h.stream));
    return SFL_OK;
}

template <class H>
int trail_start(H *x, int every, int capacity, const char *call)
{
    if (every < 1) return fail(SFL_ERR_INVALID, "%s: every must be >= 1 (got %d)", call, every);
    if (capacity < 1) return fail(SFL_ERR_INVALID, "%s: capacity must be >= 1 (got %d)", call, capacity);
    SFL_TRY(check_handle(x, call));
    const Holder h = holder_of(x);
    TracerSet &t = *h.t;
    if (t.count == 0) return fail(SFL_ERR_STATE, "%s: no tracers attached: a trail needs a set (sfl_tracers_set, sfl_batch_tracers_set)", call);
    const size_t slot_bytes = slot_floats(h) * sizeof(float);
    if ((size_t)capacity > SIZE_MAX / slot_bytes)
        return fail(SFL_ERR_INVALID, "%s: capacity %d slots of %zu bytes each exceed the address space", call, capacity, slot_bytes);
    HIP_TRY(hipSetDevice(h.device));
    if (t.d_trail && capacity > t.capacity) {   // an advance may still write the old slots: drain on growth only
        HIP_TRY(hipStreamSynchronize(h.stream));
        (void)hipFree(t.d_trail);
        t.d_trail = nullptr;
    }
    t.trail_on = false;   // no trail unless the slots are there
    t.every = t.capacity = t.written = 0;
    t.advances = 0;
    if (!t.d_trail) {
        void *mem = nullptr;
        HIP_TRY(hipMalloc(&mem, (size_t)capacity * slot_bytes));
        t.d_trail = static_cast<float *>(mem);
    }
    t.trail_on = true;
    t.every = every;
    t.capacity = capacity;
    return SFL_OK;
}

template <class H>
int trail_stop(H *x, const char *call)
{
    SFL_TRY(check_handle(x, call));
    const Holder h = holder_of(x);
    TracerSet &t = *h.t;
    t.trail_on = false;
    t.every = t.capacity = t.written = 0;
    t.advances = 0;
    if (!t.d_trail) return SFL_OK;
    HIP_TRY(hipSetDevice(h.device));
    HIP_TRY(hipStreamSynchronize(h.stream));   // an advance may still write the slots
    (void)hipFree(t.d_trail);
    t.d_trail = nullptr;
    return SFL_OK;
}

template <class H>
int trail_info(H *x, int *written, int *capacity, int64_t *advances, const char *call)
{
    SFL_TRY(check_handle(x, call));
    const TracerSet &t = *holder_of(x).t;
    if (written) *written = t.written;
    if (capacity) *capacity = t.capacity;
    if (advances) *advances = t.advances;
    return SFL_OK;
}

template <class H>
int trail_read(H *x, int first_slot, int slots, float *xy, size_t capacity, const char *call)
{
    if (first_slot < 0 || slots < 0) return fail(SFL_ERR_INVALID, "%s: slots [%d, %d + %d): first_slot and slots must be >= 0", call, first_slot, first_slot, slots);
    SFL_TRY(check_handle(x, call));
    const Holder h = holder_of(x);
    const TracerSet &t = *h.t;
    if (!t.trail_on) return fail(SFL_ERR_STATE, "%s: no trail to read: call sfl_tracers_trail_start (sfl_batch_tracers_trail_start) first", call);
    if ((int64_t)first_slot + slots > t.written)
        return fail(SFL_ERR_INVALID, "%s: slots [%d, %d + %d) are not inside the %d slots written so far, [0, %d)", call, first_slot, first_slot,
                    slots, t.written, t.written);
    const size_t floats = (size_t)slots * slot_floats(h);
    if (capacity < floats) return fail(SFL_ERR_INVALID, "%s: %d slots are %zu floats, capacity is %zu", call, slots, floats, capacity);
    if (slots == 0) return SFL_OK;
    if (!xy) return fail(SFL_ERR_INVALID, "%s: NULL argument", call);
    HIP_TRY(hipSetDevice(h.device));
    HIP_TRY(hipMemcpyAsync(xy, t.d_trail + (size_t)first_slot * slot_floats(h), floats * sizeof(float), hipMemcpyDeviceToHost, h.stream));
    HIP_TRY(hipStreamSynchronize(h.stream));
    return SFL_OK;
}

}  // namespace

extern "C" {

int sfl_tracers_set(sfl_context *ctx, const float *xy, size_t n, int follow)
{
    SFL_TRY(check_handle(ctx, "sfl_tracers_set"));
    const int rc = set(holder_of(ctx), xy, n, follow);   // (a refused call leaves the set, and so the hook, as they were)
    ctx->tracers_follow = ctx->tracers.count && ctx->tracers.follow ? follow_context : nullptr;
    return rc;
}

int sfl_tracers_count(sfl_context *ctx, size_t *n)
{
    if (!ctx || !n) return fail(SFL_ERR_INVALID, "sfl_tracers_count: NULL argument");
    *n = ctx->tracers.count;
    return SFL_OK;
}

int sfl_tracers_download(sfl_context *ctx, float *xy, size_t capacity)
{
    SFL_TRY(check_handle(ctx, "sfl_tracers_download"));
    return download(holder_of(ctx), xy, capacity, "sfl_tracers_download");
}

int sfl_tracers_advance(sfl_context *ctx, float dt) { return advance_now(ctx, dt, "sfl_tracers_advance"); }

int sfl_tracers_sample(sfl_context *ctx, int field, int no_slip, void *out, size_t capacity_bytes)
{
    return sample_now(ctx, field, no_slip, out, capacity_bytes, "sfl_tracers_sample");
}

int sfl_tracers_trail_start(sfl_context *ctx, int every, int capacity) { return trail_start(ctx, every, capacity, "sfl_tracers_trail_start"); }
int sfl_tracers_trail_stop(sfl_context *ctx) { return trail_stop(ctx, "sfl_tracers_trail_stop"); }
int sfl_tracers_trail_info(sfl_context *ctx, int *written, int *capacity, int64_t *advances)
{
    return trail_info(ctx, written, capacity, advances, "sfl_tracers_trail_info");
}
int sfl_tracers_trail_read(sfl_context *ctx, int first_slot, int slots, float *xy, size_t capacity)
{
    return trail_read(ctx, first_slot, slots, xy, capacity, "sfl_tracers_trail_read");
}

int sfl_batch_tracers_set(sfl_batch *b, const float *xy, size_t k, int follow)
{
    SFL_TRY(check_handle(b, "sfl_batch_tracers_set"));
    const int rc = set(holder_of(b), xy, k, follow);   // (a refused call leaves the set, and so the hook, as they were)
    b->tracers_follow = b->tracers.count && b->tracers.follow ? follow_batch : nullptr;
    return rc;
}

int sfl_batch_tracers_count(sfl_batch *b, size_t *k)
{
    if (!b || !k) return fail(SFL_ERR_INVALID, "sfl_batch_tracers_count: NULL argument");
    *k = b->tracers.count;
    return SFL_OK;
}

int sfl_batch_tracers_download(sfl_batch *b, float *xy, size_t capacity)
{
    SFL_TRY(check_handle(b, "sfl_batch_tracers_download"));
    return download(holder_of(b), xy, capacity, "sfl_batch_tracers_download");
}

int sfl_batch_tracers_advance(sfl_batch *b, float dt) { return advance_now(b, dt, "sfl_batch_tracers_advance"); }

int sfl_batch_tracers_sample(sfl_batch *b, int field, int no_slip, void *out, size_t capacity_bytes)
{
    return sample_now(b, field, no_slip, out, capacity_bytes, "sfl_batch_tracers_sample");
}

int sfl_batch_tracers_trail_start(sfl_batch *b, int every, int capacity) { return trail_start(b, every, capacity, "sfl_batch_tracers_trail_start"); }
int sfl_batch_tracers_trail_stop(sfl_batch *b) { return trail_stop(b, "sfl_batch_tracers_trail_stop"); }
int sfl_batch_tracers_trail_info(sfl_batch *b, int *written, int *capacity, int64_t *advances)
{
    return trail_info(b, written, capacity, advances, "sfl_batch_tracers_trail_info");
}
int sfl_batch_tracers_trail_read(sfl_batch *b, int first_slot, int slots, float *xy, size_t capacity)
{
    return trail_read(b, first_slot, slots, xy, capacity, "sfl_batch_tracers_trail_read");
}

}  // extern "C"
