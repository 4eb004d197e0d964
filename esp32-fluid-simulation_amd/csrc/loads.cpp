// loads.cpp -- loads (include/sfl.h "LOADS"; sfl_batch_set_bodies, sfl_batch_loads, sfl_batch_loads_* of a batch,
// sfl_set_bodies, sfl_loads, sfl_loads_* of a whole-domain context): the pressure force on solid bodies, as figures from the
// pressure held and as curves sampled on the stream between the step launches.  Host C++ only; a batch's sample is ONE
// launch of loads.hip (load_kernels.h), a context's a memset and two.
//
// The step calls live in units that the host test harnesses link without this one, so they do not call into it: the
// labels and the recorder are plain data on the two structs (context.h Loads; freed by the destroy paths, the recorder's
// room checked by the step calls themselves through loads_admit), and the sample is reached through their `loads_step`
// pointer, set here while a recorder is on and null otherwise -- then a step call launches exactly what it launched before
// there were loads.  The recorder's calls are body_recorder.h's, which friction.cpp uses for its own; the labels and the
// number of bodies stay here, and sfl_[batch_]set_bodies is refused while either recorder is on.
#include "body_recorder.h"
#include "load_kernels.h"

using namespace sfl::host;
using namespace sfl::host::body_recorder;

static_assert(sizeof(struct sfl_body_load) == 48 && offsetof(struct sfl_body_load, fy) == 8 && offsetof(struct sfl_body_load, exp2) == 16 &&
                  offsetof(struct sfl_body_load, max_abs_p) == 20 && offsetof(struct sfl_body_load, faces) == 24 &&
                  offsetof(struct sfl_body_load, nonfinite) == 40 && offsetof(struct sfl_body_load, reserved) == 44,
              "sfl_body_load: 48 bytes, offsets 0 8 16 20 24 40 44");

namespace {

int step_batch(sfl_batch *b, int steps);
int step_context(sfl_context *c);

// the loads as a kind of body_recorder.h: the calls themselves (start, stop, info, read, the figures at once) live there
struct LoadsKind : ZeroRecords<struct sfl_body_load> {
    typedef struct sfl_body_load Record;
    static constexpr const char *kNoun = "loads", *kRecorder = "loads recorder", *kStartCalls = "sfl_loads_start (sfl_batch_loads_start)";
    static Loads &state(sfl_context *c) { return c->loads; }
    static Loads &state(sfl_batch *b) { return b->loads; }
    static void set_hook(sfl_context *c) { c->loads_step = c->loads.on ? step_context : nullptr; }
    static void set_hook(sfl_batch *b) { b->loads_step = b->loads.on ? step_batch : nullptr; }

    // the records of members [first, first + count) from the fields held, into out: launches only (solids are set)
    static int launch_sample(sfl_batch *b, int first, int count, struct sfl_body_load *out)
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
    static int launch_sample(sfl_context *c, int, int, struct sfl_body_load *out)
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
};
typedef LoadsKind K;

int step_batch(sfl_batch *b, int steps) { return step<K>(b, steps); }
int step_context(sfl_context *c) { return step<K>(c, 1); }

bool friction_on(const sfl_context *c) { return c->friction.on; }
bool friction_on(const sfl_batch *b) { return b->friction.on; }
Torque &torque_of(sfl_context *c) { return c->torque; }
Torque &torque_of(sfl_batch *b) { return b->torque; }

template <class H>
int set_bodies(H *x, const uint8_t *labels, int per_member, int bodies, const char *call)
{
    if (per_member != 0 && per_member != 1) return fail(SFL_ERR_INVALID, "%s: per_member must be 0 or 1 (got %d)", call, per_member);
    if (labels && (bodies < 1 || bodies > SFL_MAX_BODIES))
        return fail(SFL_ERR_INVALID, "%s: bodies must be 1..%d (got %d)", call, SFL_MAX_BODIES, bodies);
    SFL_TRY(check_handle(x, call, K::kNoun, labels != nullptr));
    const Holder o = holder_of(x);
    Loads &l = K::state(x);
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
    if (friction_on(x))
        return fail(SFL_ERR_STATE, "%s: the friction recorder is on and the layout of its samples depends on the number of bodies: nothing set; "
                    "stop it first (sfl_friction_stop, sfl_batch_friction_stop)", call);
    if (torque_of(x).on)
        return fail(SFL_ERR_STATE, "%s: the torque recorder is on and the layout of its samples depends on the number of bodies: nothing set; "
                    "stop it first (sfl_torque_stop, sfl_batch_torque_stop)", call);
    HIP_TRY(hipSetDevice(o.device));
    HIP_TRY(hipStreamSynchronize(o.stream));   // a sample in flight may still read the bytes this call replaces
    if ((labels ? bodies : 1) != l.bodies) {   // the pivots are per body: another number of bodies puts them back to (0, 0)
        Torque &t = torque_of(x);
        if (t.d_pivot2) (void)hipFree(t.d_pivot2);
        t.d_pivot2 = nullptr;
        t.d_pivot_bytes = 0;
        t.pivots_per_member = false;
        t.h_pivot2.clear();
    }
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
    SFL_TRY(check_handle(x, call, K::kNoun));
    const Holder o = holder_of(x);
    const Loads &l = K::state(x);
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

}  // namespace

extern "C" {

int sfl_batch_set_bodies(sfl_batch *b, const uint8_t *labels, int per_member, int bodies)
{
    return set_bodies(b, labels, per_member, bodies, "sfl_batch_set_bodies");
}
int sfl_batch_bodies_info(sfl_batch *b, int *bodies, int *labelled, int *per_member)
{
    SFL_TRY(check_handle(b, "sfl_batch_bodies_info", K::kNoun));
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
    return now<K>(b, first, count, host, bytes, "sfl_batch_loads");
}
int sfl_batch_loads_start(sfl_batch *b, int every, int first, int count, int capacity)
{
    return start<K>(b, every, first, count, capacity, "sfl_batch_loads_start");
}
int sfl_batch_loads_stop(sfl_batch *b) { return stop<K>(b, "sfl_batch_loads_stop"); }
int sfl_batch_loads_info(sfl_batch *b, int *samples, int *capacity, int64_t *steps, int *bodies)
{
    return info<K>(b, samples, capacity, steps, bodies, "sfl_batch_loads_info");
}
int sfl_batch_loads_read(sfl_batch *b, int first_sample, int samples, struct sfl_body_load *host, size_t bytes)
{
    return read<K>(b, first_sample, samples, host, bytes, "sfl_batch_loads_read");
}

int sfl_set_bodies(sfl_context *ctx, const uint8_t *labels, int bodies) { return set_bodies(ctx, labels, 0, bodies, "sfl_set_bodies"); }
int sfl_bodies_info(sfl_context *ctx, int *bodies, int *labelled)
{
    SFL_TRY(check_handle(ctx, "sfl_bodies_info", K::kNoun, false));
    if (bodies) *bodies = ctx->loads.bodies;
    if (labelled) *labelled = ctx->loads.d_labels ? 1 : 0;
    return SFL_OK;
}
int sfl_bodies_download(sfl_context *ctx, uint8_t *host, size_t bytes) { return bodies_download(ctx, 0, 1, host, bytes, "sfl_bodies_download"); }
int sfl_loads(sfl_context *ctx, struct sfl_body_load *host, size_t bytes) { return now<K>(ctx, 0, 1, host, bytes, "sfl_loads"); }
int sfl_loads_start(sfl_context *ctx, int every, int capacity) { return start<K>(ctx, every, 0, 1, capacity, "sfl_loads_start"); }
int sfl_loads_stop(sfl_context *ctx) { return stop<K>(ctx, "sfl_loads_stop"); }
int sfl_loads_info(sfl_context *ctx, int *samples, int *capacity, int64_t *steps, int *bodies)
{
    return info<K>(ctx, samples, capacity, steps, bodies, "sfl_loads_info");
}
int sfl_loads_read(sfl_context *ctx, int first_sample, int samples, struct sfl_body_load *host, size_t bytes)
{
    return read<K>(ctx, first_sample, samples, host, bytes, "sfl_loads_read");
}

}  // extern "C"
