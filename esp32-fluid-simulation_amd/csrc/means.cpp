// means.cpp -- averages (include/sfl.h "AVERAGES"; sfl_batch_mean_* of a batch of either kind, sfl_mean_* of a whole-domain
// context): per-cell sums over time of the velocity, its second moments, the pressure and the dye, added on the stream
// between the step launches and downloaded afterwards.  Host C++ only; a sample is ONE launch of means.hip (mean_kernels.h).
//
// A unit of its own, as history.cpp is and for the same reason: the step calls live in units that the host test harnesses
// link without this one, so they do not call into it.  The averages are plain data on the two structs (context.h Means; freed
// by the destroy paths, the cut points of a replay found by the step calls themselves through mean_run) and the sample is
// reached through their `mean_step` pointer, set here while averages are on with every >= 1 and null otherwise -- then a
// step call launches exactly what it launched before there were averages.
#include "batch_state.h"
#include "mean_kernels.h"

using namespace sfl::host;

static_assert(SFL_MEAN_PLANES == 10 && SFL_MEAN_ALL == (SFL_MEAN_VELOCITY | SFL_MEAN_STRESS | SFL_MEAN_PRESSURE | SFL_MEAN_DYE),
              "ten planes in four groups");

namespace {

constexpr size_t kValue = 8;   // bytes of a plane's value: a double, or a uint64 of the dye
// the group of every plane id
constexpr unsigned kGroupOf[SFL_MEAN_PLANES] = {SFL_MEAN_VELOCITY, SFL_MEAN_VELOCITY, SFL_MEAN_STRESS,   SFL_MEAN_STRESS, SFL_MEAN_STRESS,
                                                SFL_MEAN_PRESSURE, SFL_MEAN_PRESSURE, SFL_MEAN_DYE,      SFL_MEAN_DYE,    SFL_MEAN_DYE};

int planes_of(unsigned what)
{
    int n = 0;
    for (int k = 0; k < SFL_MEAN_PLANES; ++k) n += (what & kGroupOf[k]) ? 1 : 0;
    return n;
}
// where plane `plane` lies among the live ones of `what`
int slot_of(unsigned what, int plane)
{
    int n = 0;
    for (int k = 0; k < plane; ++k) n += (what & kGroupOf[k]) ? 1 : 0;
    return n;
}

struct Holder {
    Means *m;
    hipStream_t stream;
    int device, members;
    size_t cells;   // of one member
    bool batch;
};
Holder holder_of(sfl_context *c) { return Holder{&c->means, c->stream, c->device, 1, (size_t)c->dim_x * c->gdim_y, false}; }
Holder holder_of(sfl_batch *b) { return Holder{&b->means, b->stream, b->device, b->batch, b->cells, true}; }

// (`whole`: the call needs a whole-domain context without a transport, as sfl_set_solids does)
int check_handle(sfl_context *c, const char *call, bool whole = true)
{
    if (!c) return fail(SFL_ERR_INVALID, "%s: ctx is NULL", call);
    if (whole && c->nranks != 1)
        return fail(SFL_ERR_STATE, "%s: whole-domain contexts only (slab %d/%d): a slab's planes would need the ranks' rows put together", call,
                    c->rank, c->nranks);
    if (whole && c->transport) return fail(SFL_ERR_STATE, "%s: the context has a transport attached: it keeps no averages", call);
    return SFL_OK;
}
int check_handle(sfl_batch *b, const char *call, bool = true)
{
    if (!b) return fail(SFL_ERR_INVALID, "%s: batch is NULL", call);
    return SFL_OK;
}

double *plane_ptr(const Means &m, int plane)
{
    return static_cast<double *>(m.d_planes) + (size_t)slot_of(m.what, plane) * m.count * m.member_stride;
}

// the fields held, as the sample reads them
int fields_of(sfl_batch *b, sfl::MeanSample *a)
{
    a->v = b->vel;
    a->p = b->p;
    a->dye = b->col;
    return SFL_OK;
}
int fields_of(sfl_context *c, sfl::MeanSample *a)
{
    const unsigned what = c->means.what;
    if (what & (SFL_MEAN_VELOCITY | SFL_MEAN_STRESS)) SFL_TRY(ensure_field(c, SFL_FIELD_VELOCITY));
    if (what & SFL_MEAN_PRESSURE) SFL_TRY(ensure_field(c, SFL_FIELD_PRESSURE));
    if (what & SFL_MEAN_DYE) SFL_TRY(ensure_field(c, SFL_FIELD_COLOR));
    SFL_TRY(use_device(c));
    a->v = c->vel;   // (a whole-domain context has no ghost rows: its arrays are the domain's)
    a->p = c->p;
    a->dye = c->col;
    return SFL_OK;
}

// one sample of the fields held, on the stream
template <class H>
int add_sample(H *x)
{
    const Holder o = holder_of(x);
    Means &m = *o.m;
    sfl::MeanSample a{};
    SFL_TRY(fields_of(x, &a));
    a.cells = o.cells;
    a.member_stride = m.member_stride;
    a.first = m.first;
    a.count = m.count;
    a.what = m.what;
    for (int k = 0; k < SFL_MEAN_PLANES; ++k) a.plane[k] = (m.what & kGroupOf[k]) ? plane_ptr(m, k) : nullptr;
    HIP_TRY(sfl::launch_mean_sample(o.stream, a));
    ++m.samples;
    return SFL_OK;
}

// `steps` steps have run in one launch (mean_run saw to it that no sample falls inside them): count them
template <class H>
int step(H *x, int steps)
{
    Means &m = *holder_of(x).m;
    m.steps += steps;
    return m.steps % m.every == 0 ? add_sample(x) : SFL_OK;
}
int step_batch(sfl_batch *b, int steps) { return step(b, steps); }
int step_context(sfl_context *c) { return step(c, 1); }

void set_hook(sfl_context *c) { c->mean_step = c->means.on && c->means.every > 0 ? step_context : nullptr; }
void set_hook(sfl_batch *b) { b->mean_step = b->means.on && b->means.every > 0 ? step_batch : nullptr; }

// frees the planes behind the work in flight; the state goes first, so that a failure leaves no averages
template <class H>
int release(H *x, const Holder &o)
{
    void *planes = o.m->d_planes;
    *o.m = Means{};
    set_hook(x);
    if (!planes) return SFL_OK;
    HIP_TRY(hipSetDevice(o.device));
    HIP_TRY(hipStreamSynchronize(o.stream));   // a sample may still write the planes
    (void)hipFree(planes);
    return SFL_OK;
}

template <class H>
int start(H *x, int what, int every, int first, int count, const char *call)
{
    if (what < 1 || what > SFL_MEAN_ALL)
        return fail(SFL_ERR_INVALID, "%s: what must be a mask of SFL_MEAN_* groups, 1..%d (got %d)", call, SFL_MEAN_ALL, what);
    if (every < 0) return fail(SFL_ERR_INVALID, "%s: every must be >= 0 (got %d)", call, every);
    if (count < 1) return fail(SFL_ERR_INVALID, "%s: count must be >= 1 (got %d)", call, count);
    SFL_TRY(check_handle(x, call));
    const Holder o = holder_of(x);
    if (first < 0 || (int64_t)first + count > o.members)
        return fail(SFL_ERR_INVALID, "%s: members [%d, %d + %d) are not inside the batch's [0, %d)", call, first, first, count, o.members);
    SFL_TRY(release(x, o));   // a start while on begins anew: no averages unless the planes are there
    const size_t stride = sfl::mean_member_stride(o.cells);
    const size_t bytes = (size_t)planes_of((unsigned)what) * count * stride * kValue;   // < 10 * 2^31 * 2^28 * 8
    HIP_TRY(hipSetDevice(o.device));
    void *planes = nullptr;
    const hipError_t e = hipMalloc(&planes, bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();   // (so that the next launch's check does not report this failure again)
        return fail(e == hipErrorOutOfMemory ? SFL_ERR_NOMEM : SFL_ERR_HIP, "%s: hipMalloc of %zu bytes of planes (%d planes of %d x %zu values) failed: %s",
                    call, bytes, planes_of((unsigned)what), count, stride, hipGetErrorString(e));
    }
    const hipError_t z = hipMemsetAsync(planes, 0, bytes, o.stream);   // +0.0 and 0 are zero bytes
    if (z != hipSuccess) {
        (void)hipFree(planes);
        return fail(SFL_ERR_HIP, "%s: hipMemsetAsync of %zu bytes of planes failed: %s", call, bytes, hipGetErrorString(z));
    }
    Means &m = *o.m;
    m.on = true;
    m.what = (unsigned)what;
    m.every = every;
    m.first = first;
    m.count = count;
    m.d_planes = planes;
    m.member_stride = stride;
    m.d_bytes = bytes;
    set_hook(x);
    return SFL_OK;
}

template <class H>
int stop(H *x, const char *call)
{
    SFL_TRY(check_handle(x, call, false));
    return release(x, holder_of(x));
}

template <class H>
int sample(H *x, const char *call)
{
    SFL_TRY(check_handle(x, call));
    if (!holder_of(x).m->on)
        return fail(SFL_ERR_STATE, "%s: no averages to add to: call sfl_mean_start (sfl_batch_mean_start) first", call);
    return add_sample(x);
}

template <class H>
int info(H *x, int *what, int *every, int64_t *samples, int64_t *steps, const char *call)
{
    SFL_TRY(check_handle(x, call, false));
    const Means &m = *holder_of(x).m;
    if (what) *what = (int)m.what;
    if (every) *every = m.every;
    if (samples) *samples = m.samples;
    if (steps) *steps = m.steps;
    return SFL_OK;
}

template <class H>
int download(H *x, int plane, int first, int count, void *host, size_t bytes, const char *call)
{
    if (plane < 0 || plane >= SFL_MEAN_PLANES)
        return fail(SFL_ERR_INVALID, "%s: plane must be one of SFL_MEAN_PLANE_*, 0..%d (got %d)", call, SFL_MEAN_PLANES - 1, plane);
    if (count < 1) return fail(SFL_ERR_INVALID, "%s: members must be >= 1 (got %d)", call, count);
    SFL_TRY(check_handle(x, call));
    const Holder o = holder_of(x);
    const Means &m = *o.m;
    const size_t want = (size_t)count * o.cells * kValue;
    if (bytes != want && o.batch)
        return fail(SFL_ERR_INVALID, "%s: a plane of %d members of %zu values of 8 bytes is %zu bytes, got %zu", call, count, o.cells, want, bytes);
    if (bytes != want) return fail(SFL_ERR_INVALID, "%s: a plane of %zu values of 8 bytes is %zu bytes, got %zu", call, o.cells, want, bytes);
    if (!m.on) return fail(SFL_ERR_STATE, "%s: no averages to download: call sfl_mean_start (sfl_batch_mean_start) first", call);
    if (!(m.what & kGroupOf[plane]))
        return fail(SFL_ERR_INVALID, "%s: plane %d belongs to group %u, which is not in the mask %u the averages were started with", call, plane,
                    kGroupOf[plane], m.what);
    if (first < m.first || (int64_t)first + count > (int64_t)m.first + m.count)
        return fail(SFL_ERR_INVALID, "%s: members [%d, %d + %d) are not inside the recorded [%d, %d + %d)", call, first, first, count, m.first,
                    m.first, m.count);
    if (!host) return fail(SFL_ERR_INVALID, "%s: host is NULL", call);
    HIP_TRY(hipSetDevice(o.device));
    const double *dev = plane_ptr(m, plane) + (size_t)(first - m.first) * m.member_stride;
    if (m.member_stride == o.cells || count == 1)   // dense on the device too: one copy
        HIP_TRY(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, o.stream));
    else   // a member's cells are a row of a pitched array
        HIP_TRY(hipMemcpy2DAsync(host, o.cells * kValue, dev, m.member_stride * kValue, o.cells * kValue, (size_t)count, hipMemcpyDeviceToHost,
                                 o.stream));
    HIP_TRY(hipStreamSynchronize(o.stream));
    return SFL_OK;
}

}  // namespace

extern "C" {

int sfl_batch_mean_start(sfl_batch *b, int what, int every, int first, int count)
{
    return start(b, what, every, first, count, "sfl_batch_mean_start");
}
int sfl_batch_mean_stop(sfl_batch *b) { return stop(b, "sfl_batch_mean_stop"); }
int sfl_batch_mean_sample(sfl_batch *b) { return sample(b, "sfl_batch_mean_sample"); }
int sfl_batch_mean_info(sfl_batch *b, int *what, int *every, int64_t *samples, int64_t *steps)
{
    return info(b, what, every, samples, steps, "sfl_batch_mean_info");
}
int sfl_batch_mean_download(sfl_batch *b, int plane, int first_member, int members, void *host, size_t bytes)
{
    return download(b, plane, first_member, members, host, bytes, "sfl_batch_mean_download");
}

int sfl_mean_start(sfl_context *ctx, int what, int every) { return start(ctx, what, every, 0, 1, "sfl_mean_start"); }
int sfl_mean_stop(sfl_context *ctx) { return stop(ctx, "sfl_mean_stop"); }
int sfl_mean_sample(sfl_context *ctx) { return sample(ctx, "sfl_mean_sample"); }
int sfl_mean_info(sfl_context *ctx, int *what, int *every, int64_t *samples, int64_t *steps)
{
    return info(ctx, what, every, samples, steps, "sfl_mean_info");
}
int sfl_mean_download(sfl_context *ctx, int plane, void *host, size_t bytes) { return download(ctx, plane, 0, 1, host, bytes, "sfl_mean_download"); }

}  // extern "C"
