// loads.cpp -- loads (include/sfl.h "LOADS"; sfl_batch_set_bodies, sfl_batch_loads, sfl_batch_loads_* of a batch,
// sfl_set_bodies, sfl_loads, sfl_loads_* of a whole-domain context): the pressure force on solid bodies, as figures from the
// pressure held and as curves sampled on the stream between the step launches.  Host C++ only; a batch's sample is ONE
// launch of loads.hip (load_kernels.h), a context's a memset and two.
//
// The step calls live in units that the host test harnesses link without this one, so they do not call into it: the
// labels and the recorder are plain data on the two structs (context.h Loads; freed by the destroy paths, the recorder's
// room checked by the step calls themselves through loads_admit), and the sample is reached through their `loads_step`
// pointer, set here while a recorder is on and null otherwise -- then a step call launches exactly what it launched before
// there were loads.
#include "batch_state.h"
#include "load_kernels.h"

using namespace sfl::host;

static_assert(sizeof(struct sfl_body_load) == 48 && offsetof(struct sfl_body_load, fy) == 8 && offsetof(struct sfl_body_load, exp2) == 16 &&
                  offsetof(struct sfl_body_load, max_abs_p) == 20 && offsetof(struct sfl_body_load, faces) == 24 &&
                  offsetof(struct sfl_body_load, nonfinite) == 40 && offsetof(struct sfl_body_load, reserved) == 44,
              "sfl_body_load: 48 bytes, offsets 0 8 16 20 24 40 44");

namespace {

constexpr size_t kRecord = sizeof(struct sfl_body_load);

struct Holder {
    Loads *l;
    hipStream_t stream;
    int device, members, dim_x, dim_y;
    bool solids, batch;   // batch: the messages speak of members
};
Holder holder_of(sfl_context *c) { return Holder{&c->loads, c->stream, c->device, 1, c->dim_x, c->gdim_y, c->solids.set, false}; }
Holder holder_of(sfl_batch *b) { return Holder{&b->loads, b->stream, b->device, b->batch, b->dim_x, b->dim_y, b->solids.set, true}; }

// (`whole`: the call needs a whole-domain context without a transport, as sfl_set_solids does)
int check_handle(sfl_context *c, const char *call, bool whole = true)
{
    if (!c) return fail(SFL_ERR_INVALID, "%s: ctx is NULL", call);
    if (whole && c->nranks != 1)
        return fail(SFL_ERR_STATE, "%s: whole-domain contexts only (slab %d/%d): a slab has no solid cells and no loads", call, c->rank, c->nranks);
    if (whole && c->transport)
        return fail(SFL_ERR_STATE, "%s: the context has a transport attached: it has no solid cells and no loads", call);
    return SFL_OK;
}
int check_handle(sfl_batch *b, const char *call, bool = true)
{
    if (!b) return fail(SFL_ERR_INVALID, "%s: batch is NULL", call);
    return SFL_OK;
}

size_t scratch_records(const Holder &o) { return (size_t)o.members * o.l->bodies; }
struct sfl_body_load *records(const Loads &l) { return static_cast<struct sfl_body_load *>(l.d_records); }
struct sfl_body_load *slot(const Holder &o, int sample)
{
    return records(*o.l) + scratch_records(o) + (size_t)sample * o.l->count * o.l->bodies;
}

// d_records holds at least `bytes`: kept when it does, else drained (a sample may still write it) and made anew
int ensure_records(const Holder &o, size_t bytes, const char *call)
{
    Loads &l = *o.l;
    if (l.d_records && l.d_bytes >= bytes) return SFL_OK;
    if (l.d_records) {
        HIP_TRY(hipStreamSynchronize(o.stream));
        (void)hipFree(l.d_records);
        l.d_records = nullptr;
        l.d_bytes = 0;
    }
    void *mem = nullptr;
    const hipError_t e = hipMalloc(&mem, bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();   // (so that the next launch's check does not report this failure again)
        return fail(e == hipErrorOutOfMemory ? SFL_ERR_NOMEM : SFL_ERR_HIP, "%s: hipMalloc of %zu bytes of records failed: %s", call, bytes,
                    hipGetErrorString(e));
    }
    l.d_records = mem;
    l.d_bytes = bytes;
    return SFL_OK;
}

// the records of members [first, first + count) from the fields held, into out: launches only (solids are set)
int launch_sample(sfl_batch *b, int first, int count, struct sfl_body_load *out)
{
    const Loads &l = b->loads;
    sfl::BatchLoadSample a{};
    a.p = b->p;
    a.codes = b->solids.d_codes;
    a.code_stride = b->solids.per_member ? b->cells : 0;
    a.labels = l.d_labels;
    a.label_stride = l.per_member ? b->cells : 0;
    a.dim_x = b->dim_x;
    a.dim_y = b->dim_y;
    a.first = first;
    a.count = count;
    a.bodies = l.bodies;
    a.out = out;
    HIP_TRY(sfl::launch_batch_loads(b->stream, a));
    return SFL_OK;
}
int launch_sample(sfl_context *c, int, int, struct sfl_body_load *out)
{
    SFL_TRY(ensure_field(c, SFL_FIELD_PRESSURE));
    SFL_TRY(use_device(c));
    sfl::ContextLoadSample a{};
    a.p = c->p;
    a.codes = c->solids.d_codes;
    a.labels = c->loads.d_labels;
    a.dim_x = c->dim_x;
    a.dim_y = c->gdim_y;
    a.bodies = c->loads.bodies;
    a.out = out;
    HIP_TRY(sfl::launch_context_loads(c->stream, a));
    return SFL_OK;
}

// `steps` steps have run: count them; every sample that has come due is launched behind them -- zeroed without solids
// (a launch of several steps only runs without them, so a sample that falls inside it is zeros and needs no field)
template <class H>
int step(H *x, int steps)
{
    const Holder o = holder_of(x);
    Loads &l = *o.l;
    const int64_t before = l.steps / l.every;
    l.steps += steps;
    for (int64_t s = before; s < l.steps / l.every; ++s) {   // < capacity: loads_admit has let the call through
        struct sfl_body_load *out = slot(o, (int)s);
        if (o.solids)
            SFL_TRY(launch_sample(x, l.first, l.count, out));
        else
            HIP_TRY(hipMemsetAsync(out, 0, (size_t)l.count * l.bodies * kRecord, o.stream));
        l.written = (int)s + 1;
    }
    return SFL_OK;
}
int step_batch(sfl_batch *b, int steps) { return step(b, steps); }
int step_context(sfl_context *c) { return step(c, 1); }

void set_hook(sfl_context *c) { c->loads_step = c->loads.on ? step_context : nullptr; }
void set_hook(sfl_batch *b) { b->loads_step = b->loads.on ? step_batch : nullptr; }

void stop_recorder(Loads &l)
{
    l.on = false;
    l.every = l.first = l.count = l.capacity = l.written = 0;
    l.steps = 0;
}

template <class H>
int set_bodies(H *x, const uint8_t *labels, int per_member, int bodies, const char *call)
{
    if (per_member != 0 && per_member != 1) return fail(SFL_ERR_INVALID, "%s: per_member must be 0 or 1 (got %d)", call, per_member);
    if (labels && (bodies < 1 || bodies > SFL_MAX_BODIES))
        return fail(SFL_ERR_INVALID, "%s: bodies must be 1..%d (got %d)", call, SFL_MAX_BODIES, bodies);
    SFL_TRY(check_handle(x, call, labels != nullptr));
    const Holder o = holder_of(x);
    Loads &l = *o.l;
    const size_t cells = (size_t)o.dim_x * o.dim_y, members = per_member ? (size_t)o.members : 1, bytes = members * cells;
    for (size_t k = 0; labels && k < bytes; ++k)
        if (labels[k] > bodies) {
            const size_t c = k % cells;
            if (!o.batch) return fail(SFL_ERR_INVALID, "%s: label %d of cell (%zu, %zu) exceeds bodies = %d", call, labels[k], c % o.dim_x, c / o.dim_x, bodies);
            return fail(SFL_ERR_INVALID, "%s: label %d of cell (%zu, %zu) of member %zu exceeds bodies = %d", call, labels[k], c % o.dim_x, c / o.dim_x,
                        k / cells, bodies);
        }
    if (l.on)
        return fail(SFL_ERR_STATE, "%s: the loads recorder is on and the layout of its samples depends on the number of bodies: nothing set; "
                    "stop it first (sfl_loads_stop, sfl_batch_loads_stop)", call);
    HIP_TRY(hipSetDevice(o.device));
    HIP_TRY(hipStreamSynchronize(o.stream));   // a sample in flight may still read the bytes this call replaces
    if (!labels || bytes > l.d_label_bytes) {
        if (l.d_labels) (void)hipFree(l.d_labels);
        l.d_labels = nullptr;
        l.d_label_bytes = 0;
        l.per_member = false;
        l.bodies = 1;   // every solid cell is body 1 unless the labels are there
        if (!labels) return SFL_OK;
        void *mem = nullptr;
        const hipError_t e = hipMalloc(&mem, bytes);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(e == hipErrorOutOfMemory ? SFL_ERR_NOMEM : SFL_ERR_HIP, "%s: hipMalloc of %zu label bytes failed: %s", call, bytes,
                        hipGetErrorString(e));
        }
        l.d_labels = static_cast<uint8_t *>(mem);
        l.d_label_bytes = bytes;
    }
    HIP_TRY(hipMemcpyAsync(l.d_labels, labels, bytes, hipMemcpyHostToDevice, o.stream));
    HIP_TRY(hipStreamSynchronize(o.stream));   // (the labels are read during the call only)
    l.per_member = per_member != 0;
    l.bodies = bodies;
    return SFL_OK;
}

template <class H>
int bodies_download(H *x, int first, int count, uint8_t *host, size_t bytes, const char *call)
{
    SFL_TRY(check_handle(x, call));
    const Holder o = holder_of(x);
    const Loads &l = *o.l;
    if (first < 0 || count < 0 || (int64_t)first + count > o.members)
        return fail(SFL_ERR_INVALID, "%s: members [%d, %d + %d) are not inside the batch's [0, %d)", call, first, first, count, o.members);
    const size_t cells = (size_t)o.dim_x * o.dim_y, want = (size_t)count * cells;
    if (bytes != want && o.batch)
        return fail(SFL_ERR_INVALID, "%s: the labels of %d x %d cells of %d members are %zu bytes, got %zu", call, o.dim_x, o.dim_y, count, want, bytes);
    if (bytes != want) return fail(SFL_ERR_INVALID, "%s: the labels of %d x %d cells are %zu bytes, got %zu", call, o.dim_x, o.dim_y, want, bytes);
    if (count == 0) return SFL_OK;
    if (!host) return fail(SFL_ERR_INVALID, "%s: host is NULL", call);
    if (!l.d_labels) {   // every solid cell is body 1
        memset(host, 1, bytes);
        return SFL_OK;
    }
    HIP_TRY(hipSetDevice(o.device));
    const size_t got = l.per_member ? bytes : cells;
    HIP_TRY(hipMemcpyAsync(host, l.d_labels + (l.per_member ? (size_t)first * cells : 0), got, hipMemcpyDeviceToHost, o.stream));
    HIP_TRY(hipStreamSynchronize(o.stream));
    for (int m = 1; m < count && !l.per_member; ++m) memcpy(host + (size_t)m * cells, host, cells);
    return SFL_OK;
}

template <class H>
int loads_now(H *x, int first, int count, struct sfl_body_load *host, size_t bytes, const char *call)
{
    SFL_TRY(check_handle(x, call));
    const Holder o = holder_of(x);
    if (first < 0 || count < 0 || (int64_t)first + count > o.members)
        return fail(SFL_ERR_INVALID, "%s: members [%d, %d + %d) are not inside the batch's [0, %d)", call, first, first, count, o.members);
    const size_t want = (size_t)count * o.l->bodies * kRecord;
    if (bytes != want && o.batch)
        return fail(SFL_ERR_INVALID, "%s: %d members of %d records of 48 bytes are %zu bytes, got %zu", call, count, o.l->bodies, want, bytes);
    if (bytes != want)
        return fail(SFL_ERR_INVALID, "%s: the records of %d bodies of 48 bytes each are %zu bytes, got %zu", call, o.l->bodies, want, bytes);
    if (count == 0) return SFL_OK;
    if (!host) return fail(SFL_ERR_INVALID, "%s: host is NULL", call);
    if (!o.solids) {   // no body anywhere: no launch
        memset(host, 0, bytes);
        return SFL_OK;
    }
    HIP_TRY(hipSetDevice(o.device));
    SFL_TRY(ensure_records(o, scratch_records(o) * kRecord, call));   // (a recorder that is on has made this room)
    SFL_TRY(launch_sample(x, first, count, records(*o.l)));
    HIP_TRY(hipMemcpyAsync(host, records(*o.l), bytes, hipMemcpyDeviceToHost, o.stream));
    HIP_TRY(hipStreamSynchronize(o.stream));
    return SFL_OK;
}

template <class H>
int start(H *x, int every, int first, int count, int capacity, const char *call)
{
    if (every < 1) return fail(SFL_ERR_INVALID, "%s: every must be >= 1 (got %d)", call, every);
    if (capacity < 1) return fail(SFL_ERR_INVALID, "%s: capacity must be >= 1 (got %d)", call, capacity);
    if (count < 1) return fail(SFL_ERR_INVALID, "%s: count must be >= 1 (got %d)", call, count);
    SFL_TRY(check_handle(x, call));
    const Holder o = holder_of(x);
    Loads &l = *o.l;
    const size_t sample_bytes = (size_t)count * l.bodies * kRecord, scratch = scratch_records(o) * kRecord;   // < 2^41
    if ((size_t)capacity > (SIZE_MAX - scratch) / sample_bytes)
        return fail(SFL_ERR_INVALID, "%s: capacity %d samples of %zu bytes each exceed the address space", call, capacity, sample_bytes);
    if (first < 0 || (int64_t)first + count > o.members)
        return fail(SFL_ERR_INVALID, "%s: members [%d, %d + %d) are not inside the batch's [0, %d)", call, first, first, count, o.members);
    HIP_TRY(hipSetDevice(o.device));
    // (samples of the recorder that ends here may still be in flight: they are ahead of the new ones on the stream)
    stop_recorder(l);   // no recorder unless the samples are there
    set_hook(x);
    SFL_TRY(ensure_records(o, scratch + (size_t)capacity * sample_bytes, call));
    l.on = true;
    l.every = every;
    l.first = first;
    l.count = count;
    l.capacity = capacity;
    set_hook(x);
    return SFL_OK;
}

template <class H>
int stop(H *x, const char *call)
{
    SFL_TRY(check_handle(x, call, false));
    const Holder o = holder_of(x);
    Loads &l = *o.l;
    void *mem = l.d_records;
    stop_recorder(l);
    l.d_records = nullptr;
    l.d_bytes = 0;
    set_hook(x);
    if (!mem) return SFL_OK;
    HIP_TRY(hipSetDevice(o.device));
    HIP_TRY(hipStreamSynchronize(o.stream));   // a sample may still write the records
    (void)hipFree(mem);
    return SFL_OK;
}

template <class H>
int info(H *x, int *samples, int *capacity, int64_t *steps, int *bodies, const char *call)
{
    SFL_TRY(check_handle(x, call, false));
    const Loads &l = *holder_of(x).l;
    if (samples) *samples = l.written;
    if (capacity) *capacity = l.capacity;
    if (steps) *steps = l.steps;
    if (bodies) *bodies = l.bodies;
    return SFL_OK;
}

template <class H>
int read(H *x, int first_sample, int samples, struct sfl_body_load *host, size_t bytes, const char *call)
{
    if (first_sample < 0 || samples < 0)
        return fail(SFL_ERR_INVALID, "%s: samples [%d, %d + %d): first_sample and samples must be >= 0", call, first_sample, first_sample, samples);
    SFL_TRY(check_handle(x, call));
    const Holder o = holder_of(x);
    const Loads &l = *o.l;
    if (!l.on) return fail(SFL_ERR_STATE, "%s: no loads recorder to read: call sfl_loads_start (sfl_batch_loads_start) first", call);
    const size_t per_sample = (size_t)l.count * l.bodies, want = (size_t)samples * per_sample * kRecord;
    if (bytes != want)
        return fail(SFL_ERR_INVALID, "%s: %d samples of %zu records of 48 bytes (%d %s %d bodies) are %zu bytes, got %zu", call, samples, per_sample,
                    l.count, o.batch ? "members of" : "context of", l.bodies, want, bytes);
    if ((int64_t)first_sample + samples > l.written)
        return fail(SFL_ERR_INVALID, "%s: samples [%d, %d + %d) are not inside the %d samples written so far, [0, %d)", call, first_sample,
                    first_sample, samples, l.written, l.written);
    if (samples == 0) return SFL_OK;
    if (!host) return fail(SFL_ERR_INVALID, "%s: host is NULL", call);
    HIP_TRY(hipSetDevice(o.device));
    HIP_TRY(hipMemcpyAsync(host, slot(o, first_sample), bytes, hipMemcpyDeviceToHost, o.stream));
    HIP_TRY(hipStreamSynchronize(o.stream));
    return SFL_OK;
}

}  // namespace

extern "C" {

int sfl_batch_set_bodies(sfl_batch *b, const uint8_t *labels, int per_member, int bodies)
{
    return set_bodies(b, labels, per_member, bodies, "sfl_batch_set_bodies");
}
int sfl_batch_bodies_info(sfl_batch *b, int *bodies, int *labelled, int *per_member)
{
    SFL_TRY(check_handle(b, "sfl_batch_bodies_info"));
    if (bodies) *bodies = b->loads.bodies;
    if (labelled) *labelled = b->loads.d_labels ? 1 : 0;
    if (per_member) *per_member = b->loads.d_labels && b->loads.per_member ? 1 : 0;
    return SFL_OK;
}
int sfl_batch_bodies_download(sfl_batch *b, int first, int count, uint8_t *host, size_t bytes)
{
    return bodies_download(b, first, count, host, bytes, "sfl_batch_bodies_download");
}
int sfl_batch_loads(sfl_batch *b, int first, int count, struct sfl_body_load *host, size_t bytes)
{
    return loads_now(b, first, count, host, bytes, "sfl_batch_loads");
}
int sfl_batch_loads_start(sfl_batch *b, int every, int first, int count, int capacity)
{
    return start(b, every, first, count, capacity, "sfl_batch_loads_start");
}
int sfl_batch_loads_stop(sfl_batch *b) { return stop(b, "sfl_batch_loads_stop"); }
int sfl_batch_loads_info(sfl_batch *b, int *samples, int *capacity, int64_t *steps, int *bodies)
{
    return info(b, samples, capacity, steps, bodies, "sfl_batch_loads_info");
}
int sfl_batch_loads_read(sfl_batch *b, int first_sample, int samples, struct sfl_body_load *host, size_t bytes)
{
    return read(b, first_sample, samples, host, bytes, "sfl_batch_loads_read");
}

int sfl_set_bodies(sfl_context *ctx, const uint8_t *labels, int bodies) { return set_bodies(ctx, labels, 0, bodies, "sfl_set_bodies"); }
int sfl_bodies_info(sfl_context *ctx, int *bodies, int *labelled)
{
    SFL_TRY(check_handle(ctx, "sfl_bodies_info", false));
    if (bodies) *bodies = ctx->loads.bodies;
    if (labelled) *labelled = ctx->loads.d_labels ? 1 : 0;
    return SFL_OK;
}
int sfl_bodies_download(sfl_context *ctx, uint8_t *host, size_t bytes) { return bodies_download(ctx, 0, 1, host, bytes, "sfl_bodies_download"); }
int sfl_loads(sfl_context *ctx, struct sfl_body_load *host, size_t bytes) { return loads_now(ctx, 0, 1, host, bytes, "sfl_loads"); }
int sfl_loads_start(sfl_context *ctx, int every, int capacity) { return start(ctx, every, 0, 1, capacity, "sfl_loads_start"); }
int sfl_loads_stop(sfl_context *ctx) { return stop(ctx, "sfl_loads_stop"); }
int sfl_loads_info(sfl_context *ctx, int *samples, int *capacity, int64_t *steps, int *bodies)
{
    return info(ctx, samples, capacity, steps, bodies, "sfl_loads_info");
}
int sfl_loads_read(sfl_context *ctx, int first_sample, int samples, struct sfl_body_load *host, size_t bytes)
{
    return read(ctx, first_sample, samples, host, bytes, "sfl_loads_read");
}

}  // extern "C"
