// torque.cpp -- the torque on solid bodies (include/sfl.h "TORQUE"; sfl_batch_set_body_pivots, sfl_batch_torque,
// sfl_batch_torque_* of a batch, sfl_set_body_pivots, sfl_torque, sfl_torque_* of a whole-domain context): the moment of the
// pressure and of the tangential velocity beside the walls about a pivot per body, as figures from the fields held and as
// curves sampled on the stream between the step launches.  Host C++ only; a batch's sample is ONE launch of torque.hip
// (torque_kernels.h), a context's a memset and two.
//
// A unit of its own, as loads.cpp and friction.cpp are and for the same reason: the step calls live in units that the host
// test harnesses link against launchers of their own, so they do not call into this one.  The pivots and the recorder are
// plain data on the two structs (context.h Torque; freed by the destroy paths, the recorder's room checked by the step calls
// through torque_admit) and the sample is reached through their `torque_step` pointer, set here while a recorder is on and
// null otherwise -- then a step call launches exactly what it launched before there was a torque.  The recorder's calls are
// body_recorder.h's, shared with loads.cpp and friction.cpp; the labels and the number of bodies are the loads'
// (Loads::d_labels, ::bodies; sfl_[batch_]set_bodies, which puts the pivots back to (0, 0) when it changes the number).
#include "body_recorder.h"
#include "torque_kernels.h"

using namespace sfl::host;
using namespace sfl::host::body_recorder;

static_assert(sizeof(struct sfl_body_torque) == 64 && offsetof(struct sfl_body_torque, mf) == 8 && offsetof(struct sfl_body_torque, exp2_p) == 16 &&
                  offsetof(struct sfl_body_torque, exp2_f) == 20 && offsetof(struct sfl_body_torque, max_abs_p) == 24 &&
                  offsetof(struct sfl_body_torque, max_abs_t) == 28 && offsetof(struct sfl_body_torque, faces) == 32 &&
                  offsetof(struct sfl_body_torque, max_arm2) == 36 && offsetof(struct sfl_body_torque, nonfinite_p) == 40 &&
                  offsetof(struct sfl_body_torque, nonfinite_t) == 44 && offsetof(struct sfl_body_torque, pivot2) == 48 &&
                  offsetof(struct sfl_body_torque, reserved) == 56,
              "sfl_body_torque: 64 bytes, offsets 0 8 16 20 24 28 32 36 40 44 48 56");

namespace {

int step_batch(sfl_batch *b, int steps);
int step_context(sfl_context *c);

// the device table of the pivots as the samplers take it: null while every pivot is (0, 0) -- also when the table no longer
// fits the number of bodies (sfl_[batch_]set_bodies clears it then; this is the second lock)
struct Pivots {
    const int32_t *d;
    size_t stride;   // int32 between two members' pairs; 0: shared
};
Pivots pivots_of(const Torque &t, const Holder &o)
{
    const size_t members = t.pivots_per_member ? (size_t)o.members : 1;
    if (!t.d_pivot2 || t.h_pivot2.size() != members * o.bodies * 2) return Pivots{nullptr, 0};
    return Pivots{t.d_pivot2, t.pivots_per_member ? (size_t)o.bodies * 2 : 0};
}
// the pair of body k (from 0) of member m on the host
const int32_t *host_pivot(const Torque &t, const Holder &o, int m, int k)
{
    static const int32_t zero[2] = {0, 0};
    if (!pivots_of(t, o).d) return zero;
    return t.h_pivot2.data() + ((t.pivots_per_member ? (size_t)m * o.bodies : 0) + k) * 2;
}

struct TorqueKind {
    typedef struct sfl_body_torque Record;
    static constexpr const char *kNoun = "torque", *kRecorder = "torque recorder", *kStartCalls = "sfl_torque_start (sfl_batch_torque_start)";
    static Torque &state(sfl_context *c) { return c->torque; }
    static Torque &state(sfl_batch *b) { return b->torque; }
    static void set_hook(sfl_context *c) { c->torque_step = c->torque.on ? step_context : nullptr; }
    static void set_hook(sfl_batch *b) { b->torque_step = b->torque.on ? step_batch : nullptr; }

    // the records of members [first, first + count) from the fields held, into out: launches only (solids are set)
    static int launch_sample(sfl_batch *b, int first, int count, struct sfl_body_torque *out)
    {
        const Loads &l = b->loads;
        const Pivots pv = pivots_of(b->torque, holder_of(b));
        sfl::BatchTorqueSample a{};
        a.p = b->p;
        a.v = reinterpret_cast<const float2 *>(b->vel);
        a.codes = b->solids.d_codes;
        a.code_stride = b->solids.per_member ? b->cells : 0;
        a.labels = l.d_labels;
        a.label_stride = l.per_member ? b->cells : 0;
        a.pivot2 = pv.d;
        a.pivot_stride = pv.stride;
        a.dim_x = b->dim_x;
        a.dim_y = b->dim_y;
        a.first = first;
        a.count = count;
        a.bodies = l.bodies;
        a.out = out;
        HIP_TRY(sfl::launch_batch_torque(b->stream, a));
        return SFL_OK;
    }
    static int launch_sample(sfl_context *c, int, int, struct sfl_body_torque *out)
    {
        SFL_TRY(ensure_field(c, SFL_FIELD_PRESSURE));
        SFL_TRY(ensure_field(c, SFL_FIELD_VELOCITY));
        SFL_TRY(use_device(c));
        sfl::ContextTorqueSample a{};
        a.p = c->p;
        a.v = reinterpret_cast<const float2 *>(c->vel);
        a.codes = c->solids.d_codes;
        a.labels = c->loads.d_labels;
        a.pivot2 = pivots_of(c->torque, holder_of(c)).d;
        a.dim_x = c->dim_x;
        a.dim_y = c->gdim_y;
        a.bodies = c->loads.bodies;
        a.out = out;
        HIP_TRY(sfl::launch_context_torque(c->stream, a));
        return SFL_OK;
    }
    // no solids set: zeros and the pivots -- one small launch that reads no field, or none at all
    template <class H>
    static int zero_sample(H *x, int first, int count, struct sfl_body_torque *out)
    {
        const Holder o = holder_of(x);
        const Pivots pv = pivots_of(state(x), o);
        HIP_TRY(sfl::launch_torque_empty(o.stream, out, pv.d, pv.stride, first, count, o.bodies));
        return SFL_OK;
    }
    template <class H>
    static void zero_host(H *x, int first, int count, struct sfl_body_torque *host)
    {
        const Holder o = holder_of(x);
        memset(host, 0, (size_t)count * o.bodies * sizeof *host);
        for (int m = 0; m < count; ++m)
            for (int k = 0; k < o.bodies; ++k) memcpy(host[(size_t)m * o.bodies + k].pivot2, host_pivot(state(x), o, first + m, k), 2 * sizeof(int32_t));
    }
};
typedef TorqueKind K;

int step_batch(sfl_batch *b, int steps) { return step<K>(b, steps); }
int step_context(sfl_context *c) { return step<K>(c, 1); }

template <class H>
int set_pivots(H *x, const int32_t *pivot2, int per_member, int bodies, const char *call)
{
    if (per_member != 0 && per_member != 1) return fail(SFL_ERR_INVALID, "%s: per_member must be 0 or 1 (got %d)", call, per_member);
    SFL_TRY(check_handle(x, call, K::kNoun, pivot2 != nullptr));
    const Holder o = holder_of(x);
    Torque &t = K::state(x);
    const size_t members = per_member ? (size_t)o.members : 1, pairs = members * o.bodies, bytes = pairs * 2 * sizeof(int32_t);
    if (pivot2 && bodies != o.bodies)
        return fail(SFL_ERR_INVALID, "%s: bodies must be the %d that %s reports (got %d)", call, o.bodies, o.batch ? "sfl_batch_bodies_info" : "sfl_bodies_info", bodies);
    for (size_t k = 0; pivot2 && k < pairs * 2; ++k)
        if (pivot2[k] > SFL_TORQUE_MAX_PIVOT2 || pivot2[k] < -SFL_TORQUE_MAX_PIVOT2) {
            const size_t pair = k / 2;
            if (!o.batch || !per_member)
                return fail(SFL_ERR_INVALID, "%s: pivot2[%d] = %d of body %zu is beyond +-%d half cells", call, (int)(k % 2), pivot2[k], pair % o.bodies + 1, SFL_TORQUE_MAX_PIVOT2);
            return fail(SFL_ERR_INVALID, "%s: pivot2[%d] = %d of body %zu of member %zu is beyond +-%d half cells", call, (int)(k % 2), pivot2[k], pair % o.bodies + 1,
                        pair / o.bodies, SFL_TORQUE_MAX_PIVOT2);
        }
    HIP_TRY(hipSetDevice(o.device));
    if (!pivot2 || bytes != t.d_pivot_bytes) {   // another table: a sample in flight may still read the one that goes
        HIP_TRY(hipStreamSynchronize(o.stream));
        if (t.d_pivot2) (void)hipFree(t.d_pivot2);
        t.d_pivot2 = nullptr;
        t.d_pivot_bytes = 0;
        t.pivots_per_member = false;
        t.h_pivot2.clear();
        if (!pivot2) return SFL_OK;
        void *mem = nullptr;
        const hipError_t e = hipMalloc(&mem, bytes);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(e == hipErrorOutOfMemory ? SFL_ERR_NOMEM : SFL_ERR_HIP, "%s: hipMalloc of %zu pivot bytes failed: %s", call, bytes, hipGetErrorString(e));
        }
        t.d_pivot2 = static_cast<int32_t *>(mem);
        t.d_pivot_bytes = bytes;
    }
    // (on the stream: behind the samples that are in flight, in front of the next one)
    HIP_TRY(hipMemcpyAsync(t.d_pivot2, pivot2, bytes, hipMemcpyHostToDevice, o.stream));
    HIP_TRY(hipStreamSynchronize(o.stream));   // (the pivots are read during the call only)
    t.pivots_per_member = per_member != 0;
    t.h_pivot2.assign(pivot2, pivot2 + pairs * 2);
    return SFL_OK;
}

template <class H>
int pivots_download(H *x, int first, int count, int32_t *host, size_t bytes, const char *call)
{
    SFL_TRY(check_handle(x, call, K::kNoun));
    const Holder o = holder_of(x);
    if (first < 0 || count < 0 || (int64_t)first + count > o.members)
        return fail(SFL_ERR_INVALID, "%s: members [%d, %d + %d) are not inside the batch's [0, %d)", call, first, first, count, o.members);
    const size_t want = (size_t)count * o.bodies * 2 * sizeof(int32_t);
    if (bytes != want && o.batch)
        return fail(SFL_ERR_INVALID, "%s: the pivots of %d bodies of %d members are %zu bytes, got %zu", call, o.bodies, count, want, bytes);
    if (bytes != want) return fail(SFL_ERR_INVALID, "%s: the pivots of %d bodies are %zu bytes, got %zu", call, o.bodies, want, bytes);
    if (count == 0) return SFL_OK;
    if (!host) return fail(SFL_ERR_INVALID, "%s: host is NULL", call);
    for (int m = 0; m < count; ++m)
        for (int k = 0; k < o.bodies; ++k) memcpy(host + ((size_t)m * o.bodies + k) * 2, host_pivot(K::state(x), o, first + m, k), 2 * sizeof(int32_t));
    return SFL_OK;
}

}  // namespace

extern "C" {

int sfl_batch_set_body_pivots(sfl_batch *b, const int32_t *pivot2, int per_member, int bodies)
{
    return set_pivots(b, pivot2, per_member, bodies, "sfl_batch_set_body_pivots");
}
int sfl_batch_body_pivots_download(sfl_batch *b, int first, int count, int32_t *host, size_t bytes)
{
    return pivots_download(b, first, count, host, bytes, "sfl_batch_body_pivots_download");
}
int sfl_batch_torque(sfl_batch *b, int first, int count, struct sfl_body_torque *host, size_t bytes)
{
    return now<K>(b, first, count, host, bytes, "sfl_batch_torque");
}
int sfl_batch_torque_start(sfl_batch *b, int every, int first, int count, int capacity)
{
    return start<K>(b, every, first, count, capacity, "sfl_batch_torque_start");
}
int sfl_batch_torque_stop(sfl_batch *b) { return stop<K>(b, "sfl_batch_torque_stop"); }
int sfl_batch_torque_info(sfl_batch *b, int *samples, int *capacity, int64_t *steps, int *bodies)
{
    return info<K>(b, samples, capacity, steps, bodies, "sfl_batch_torque_info");
}
int sfl_batch_torque_read(sfl_batch *b, int first_sample, int samples, struct sfl_body_torque *host, size_t bytes)
{
    return read<K>(b, first_sample, samples, host, bytes, "sfl_batch_torque_read");
}

int sfl_set_body_pivots(sfl_context *ctx, const int32_t *pivot2, int bodies) { return set_pivots(ctx, pivot2, 0, bodies, "sfl_set_body_pivots"); }
int sfl_body_pivots_download(sfl_context *ctx, int32_t *host, size_t bytes) { return pivots_download(ctx, 0, 1, host, bytes, "sfl_body_pivots_download"); }
int sfl_torque(sfl_context *ctx, struct sfl_body_torque *host, size_t bytes) { return now<K>(ctx, 0, 1, host, bytes, "sfl_torque"); }
int sfl_torque_start(sfl_context *ctx, int every, int capacity) { return start<K>(ctx, every, 0, 1, capacity, "sfl_torque_start"); }
int sfl_torque_stop(sfl_context *ctx) { return stop<K>(ctx, "sfl_torque_stop"); }
int sfl_torque_info(sfl_context *ctx, int *samples, int *capacity, int64_t *steps, int *bodies)
{
    return info<K>(ctx, samples, capacity, steps, bodies, "sfl_torque_info");
}
int sfl_torque_read(sfl_context *ctx, int first_sample, int samples, struct sfl_body_torque *host, size_t bytes)
{
    return read<K>(ctx, first_sample, samples, host, bytes, "sfl_torque_read");
}

}  // extern "C"
