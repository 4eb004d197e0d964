// body_recorder.h -- the calls that report one record per solid body, at once and as samples recorded behind the steps,
// written once for the three kinds that exist: the loads (loads.cpp; include/sfl.h "LOADS"), the friction (friction.cpp;
// "FRICTION") and the torque (torque.cpp; "TORQUE").  Host C++ only.  Generic over the holder H (sfl_context, sfl_batch) and
// over the kind K, a struct of statics:
//     Record                        the record type (48 bytes; the torque's 64)
//     state(H *)                    the recorder's plain data on the holder (context.h Recorder, as Loads, Friction or Torque)
//     launch_sample(H *, first, count, Record *out)   the sampler's launches on the holder's stream (solids are set)
//     set_hook(H *)                 sets the holder's step pointer from state(x).on
//     zero_sample(H *, first, count, Record *out)     the records of a sample taken while no solids are set, on the stream, and
//     zero_host(H *, first, count, Record *host)      the same on the host, without a launch (ZeroRecords: all bytes zero)
//     kNoun, kRecorder, kStartCalls the words of the messages ("loads", "loads recorder", "sfl_loads_start (sfl_batch_loads_start)")
// The labels and the number of bodies are the loads' (Loads::d_labels, ::bodies) for every kind.
#pragma once
#include "batch_state.h"

namespace sfl {
namespace host {
namespace body_recorder {

struct Holder {
    hipStream_t stream;
    int device, members, dim_x, dim_y, bodies;
    bool solids, batch;   // batch: the messages speak of members
};
inline Holder holder_of(sfl_context *c) { return Holder{c->stream, c->device, 1, c->dim_x, c->gdim_y, c->loads.bodies, c->solids.set, false}; }
inline Holder holder_of(sfl_batch *b) { return Holder{b->stream, b->device, b->batch, b->dim_x, b->dim_y, b->loads.bodies, b->solids.set, true}; }

// (`whole`: the call needs a whole-domain context without a transport, as sfl_set_solids does)
inline int check_handle(sfl_context *c, const char *call, const char *noun, bool whole = true)
{
    if (!c) return fail(SFL_ERR_INVALID, "%s: ctx is NULL", call);
    if (whole && c->nranks != 1)
        return fail(SFL_ERR_STATE, "%s: whole-domain contexts only (slab %d/%d): a slab has no solid cells and no %s", call, c->rank, c->nranks, noun);
    if (whole && c->transport)
        return fail(SFL_ERR_STATE, "%s: the context has a transport attached: it has no solid cells and no %s", call, noun);
    return SFL_OK;
}
inline int check_handle(sfl_batch *b, const char *call, const char *, bool = true)
{
    if (!b) return fail(SFL_ERR_INVALID, "%s: batch is NULL", call);
    return SFL_OK;
}

// what the kinds whose records are all zeros without solids inherit
template <class R>
struct ZeroRecords {
    template <class H>
    static int zero_sample(H *x, int, int count, R *out)
    {
        const Holder o = holder_of(x);
        HIP_TRY(hipMemsetAsync(out, 0, (size_t)count * o.bodies * sizeof(R), o.stream));
        return SFL_OK;
    }
    template <class H>
    static void zero_host(H *x, int, int count, R *host) { memset(host, 0, (size_t)count * holder_of(x).bodies * sizeof(R)); }
};

inline size_t scratch_records(const Holder &o) { return (size_t)o.members * o.bodies; }
// sample `sample` of a recorder over `count` members: behind the records of one sample of every member
template <class K>
typename K::Record *slot(const Holder &o, const Recorder &l, int sample)
{
    return static_cast<typename K::Record *>(l.d_records) + scratch_records(o) + (size_t)sample * l.count * o.bodies;
}

// d_records holds at least `bytes`: kept when it does, else drained (a sample may still write it) and made anew
inline int ensure_records(const Holder &o, Recorder &l, size_t bytes, const char *call)
{
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

// `steps` steps have run: count them; every sample that has come due is launched behind them -- zeroed without solids
// (a launch of several steps only runs without them, so a sample that falls inside it is zeros and needs no field)
template <class K, class H>
int step(H *x, int steps)
{
    const Holder o = holder_of(x);
    auto &l = K::state(x);
    const int64_t before = l.steps / l.every;
    l.steps += steps;
    for (int64_t s = before; s < l.steps / l.every; ++s) {   // < capacity: the admission has let the call through
        typename K::Record *out = slot<K>(o, l, (int)s);
        if (o.solids)
            SFL_TRY(K::launch_sample(x, l.first, l.count, out));
        else
            SFL_TRY(K::zero_sample(x, l.first, l.count, out));
        l.written = (int)s + 1;
    }
    return SFL_OK;
}

inline void stop_recorder(Recorder &l)
{
    l.on = false;
    l.every = l.first = l.count = l.capacity = l.written = 0;
    l.steps = 0;
}

// the records of members [first, first + count) from the fields held, synchronously
template <class K, class H>
int now(H *x, int first, int count, typename K::Record *host, size_t bytes, const char *call)
{
    constexpr size_t kRecord = sizeof(typename K::Record);
    SFL_TRY(check_handle(x, call, K::kNoun));
    const Holder o = holder_of(x);
    auto &l = K::state(x);
    if (first < 0 || count < 0 || (int64_t)first + count > o.members)
        return fail(SFL_ERR_INVALID, "%s: members [%d, %d + %d) are not inside the batch's [0, %d)", call, first, first, count, o.members);
    const size_t want = (size_t)count * o.bodies * kRecord;
    if (bytes != want && o.batch)
        return fail(SFL_ERR_INVALID, "%s: %d members of %d records of %zu bytes are %zu bytes, got %zu", call, count, o.bodies, kRecord, want, bytes);
    if (bytes != want)
        return fail(SFL_ERR_INVALID, "%s: the records of %d bodies of %zu bytes each are %zu bytes, got %zu", call, o.bodies, kRecord, want, bytes);
    if (count == 0) return SFL_OK;
    if (!host) return fail(SFL_ERR_INVALID, "%s: host is NULL", call);
    if (!o.solids) {   // no body anywhere: no launch
        K::zero_host(x, first, count, host);
        return SFL_OK;
    }
    HIP_TRY(hipSetDevice(o.device));
    SFL_TRY(ensure_records(o, l, scratch_records(o) * kRecord, call));   // (a recorder that is on has made this room)
    typename K::Record *scratch = static_cast<typename K::Record *>(l.d_records);
    SFL_TRY(K::launch_sample(x, first, count, scratch));
    HIP_TRY(hipMemcpyAsync(host, scratch, bytes, hipMemcpyDeviceToHost, o.stream));
    HIP_TRY(hipStreamSynchronize(o.stream));
    return SFL_OK;
}

template <class K, class H>
int start(H *x, int every, int first, int count, int capacity, const char *call)
{
    constexpr size_t kRecord = sizeof(typename K::Record);
    if (every < 1) return fail(SFL_ERR_INVALID, "%s: every must be >= 1 (got %d)", call, every);
    if (capacity < 1) return fail(SFL_ERR_INVALID, "%s: capacity must be >= 1 (got %d)", call, capacity);
    if (count < 1) return fail(SFL_ERR_INVALID, "%s: count must be >= 1 (got %d)", call, count);
    SFL_TRY(check_handle(x, call, K::kNoun));
    const Holder o = holder_of(x);
    auto &l = K::state(x);
    const size_t sample_bytes = (size_t)count * o.bodies * kRecord, scratch = scratch_records(o) * kRecord;   // < 2^41
    if ((size_t)capacity > (SIZE_MAX - scratch) / sample_bytes)
        return fail(SFL_ERR_INVALID, "%s: capacity %d samples of %zu bytes each exceed the address space", call, capacity, sample_bytes);
    if (first < 0 || (int64_t)first + count > o.members)
        return fail(SFL_ERR_INVALID, "%s: members [%d, %d + %d) are not inside the batch's [0, %d)", call, first, first, count, o.members);
    HIP_TRY(hipSetDevice(o.device));
    // (samples of the recorder that ends here may still be in flight: they are ahead of the new ones on the stream)
    stop_recorder(l);   // no recorder unless the samples are there
    K::set_hook(x);
    SFL_TRY(ensure_records(o, l, scratch + (size_t)capacity * sample_bytes, call));
    l.on = true;
    l.every = every;
    l.first = first;
    l.count = count;
    l.capacity = capacity;
    K::set_hook(x);
    return SFL_OK;
}

template <class K, class H>
int stop(H *x, const char *call)
{
    SFL_TRY(check_handle(x, call, K::kNoun, false));
    const Holder o = holder_of(x);
    auto &l = K::state(x);
    void *mem = l.d_records;
    stop_recorder(l);
    l.d_records = nullptr;
    l.d_bytes = 0;
    K::set_hook(x);
    if (!mem) return SFL_OK;
    HIP_TRY(hipSetDevice(o.device));
    HIP_TRY(hipStreamSynchronize(o.stream));   // a sample may still write the records
    (void)hipFree(mem);
    return SFL_OK;
}

template <class K, class H>
int info(H *x, int *samples, int *capacity, int64_t *steps, int *bodies, const char *call)
{
    SFL_TRY(check_handle(x, call, K::kNoun, false));
    const auto &l = K::state(x);
    if (samples) *samples = l.written;
    if (capacity) *capacity = l.capacity;
    if (steps) *steps = l.steps;
    if (bodies) *bodies = holder_of(x).bodies;
    return SFL_OK;
}

template <class K, class H>
int read(H *x, int first_sample, int samples, typename K::Record *host, size_t bytes, const char *call)
{
    constexpr size_t kRecord = sizeof(typename K::Record);
    if (first_sample < 0 || samples < 0)
        return fail(SFL_ERR_INVALID, "%s: samples [%d, %d + %d): first_sample and samples must be >= 0", call, first_sample, first_sample, samples);
    SFL_TRY(check_handle(x, call, K::kNoun));
    const Holder o = holder_of(x);
    const auto &l = K::state(x);
    if (!l.on) return fail(SFL_ERR_STATE, "%s: no %s to read: call %s first", call, K::kRecorder, K::kStartCalls);
    const size_t per_sample = (size_t)l.count * o.bodies, want = (size_t)samples * per_sample * kRecord;
    if (bytes != want)
        return fail(SFL_ERR_INVALID, "%s: %d samples of %zu records of %zu bytes (%d %s %d bodies) are %zu bytes, got %zu", call, samples, per_sample,
                    kRecord, l.count, o.batch ? "members of" : "context of", o.bodies, want, bytes);
    if ((int64_t)first_sample + samples > l.written)
        return fail(SFL_ERR_INVALID, "%s: samples [%d, %d + %d) are not inside the %d samples written so far, [0, %d)", call, first_sample,
                    first_sample, samples, l.written, l.written);
    if (samples == 0) return SFL_OK;
    if (!host) return fail(SFL_ERR_INVALID, "%s: host is NULL", call);
    HIP_TRY(hipSetDevice(o.device));
    HIP_TRY(hipMemcpyAsync(host, slot<K>(o, l, first_sample), bytes, hipMemcpyDeviceToHost, o.stream));
    HIP_TRY(hipStreamSynchronize(o.stream));
    return SFL_OK;
}

}  // namespace body_recorder
}  // namespace host
}  // namespace sfl
