// friction.cpp -- the skin friction on solid bodies (include/sfl.h "FRICTION"; sfl_batch_friction, sfl_batch_friction_* of a
// batch, sfl_friction, sfl_friction_* of a whole-domain context): the tangential velocity beside the walls, as figures from
// the velocity held and as curves sampled on the stream between the step launches.  Host C++ only; a batch's sample is ONE
// launch of friction.hip (friction_kernels.h), a context's a memset and two.
//
// A unit of its own, as loads.cpp is and for the same reason: the step calls live in units that the host test harnesses
// link against launchers of their own, so they do not call into this one.  The recorder is plain data on the two structs
// (context.h Friction; freed by the destroy paths, its room checked by the step calls through friction_admit) and the
// sample is reached through their `friction_step` pointer, set here while a recorder is on and null otherwise -- then a
// step call launches exactly what it launched before there was friction.  The calls are body_recorder.h's, shared with
// loads.cpp; the labels and the number of bodies are the loads' (Loads::d_labels, ::bodies; sfl_[batch_]set_bodies).
#include "body_recorder.h"
#include "friction_kernels.h"

using namespace sfl::host;
using namespace sfl::host::body_recorder;

static_assert(sizeof(struct sfl_body_friction) == 48 && offsetof(struct sfl_body_friction, fy) == 8 && offsetof(struct sfl_body_friction, exp2) == 16 &&
                  offsetof(struct sfl_body_friction, max_abs_t) == 20 && offsetof(struct sfl_body_friction, faces) == 24 &&
                  offsetof(struct sfl_body_friction, nonfinite) == 40 && offsetof(struct sfl_body_friction, reserved) == 44,
              "sfl_body_friction: 48 bytes, the offsets of sfl_body_load: 0 8 16 20 24 40 44");

namespace {

int step_batch(sfl_batch *b, int steps);
int step_context(sfl_context *c);

struct FrictionKind : ZeroRecords<struct sfl_body_friction> {
    typedef struct sfl_body_friction Record;
    static constexpr const char *kNoun = "friction", *kRecorder = "friction recorder",
                                *kStartCalls = "sfl_friction_start (sfl_batch_friction_start)";
    static Friction &state(sfl_context *c) { return c->friction; }
    static Friction &state(sfl_batch *b) { return b->friction; }
    static void set_hook(sfl_context *c) { c->friction_step = c->friction.on ? step_context : nullptr; }
    static void set_hook(sfl_batch *b) { b->friction_step = b->friction.on ? step_batch : nullptr; }

    // the records of members [first, first + count) from the velocity held, into out: launches only (solids are set)
    static int launch_sample(sfl_batch *b, int first, int count, struct sfl_body_friction *out)
    {
        const Loads &l = b->loads;
        sfl::BatchFrictionSample a{};
        a.v = reinterpret_cast<const float2 *>(b->vel);
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
        HIP_TRY(sfl::launch_batch_friction(b->stream, a));
        return SFL_OK;
    }
    static int launch_sample(sfl_context *c, int, int, struct sfl_body_friction *out)
    {
        SFL_TRY(ensure_field(c, SFL_FIELD_VELOCITY));
        SFL_TRY(use_device(c));
        sfl::ContextFrictionSample a{};
        a.v = reinterpret_cast<const float2 *>(c->vel);
        a.codes = c->solids.d_codes;
        a.labels = c->loads.d_labels;
        a.dim_x = c->dim_x;
        a.dim_y = c->gdim_y;
        a.bodies = c->loads.bodies;
        a.out = out;
        HIP_TRY(sfl::launch_context_friction(c->stream, a));
        return SFL_OK;
    }
};
typedef FrictionKind K;

int step_batch(sfl_batch *b, int steps) { return step<K>(b, steps); }
int step_context(sfl_context *c) { return step<K>(c, 1); }

}  // namespace

extern "C" {

int sfl_batch_friction(sfl_batch *b, int first, int count, struct sfl_body_friction *host, size_t bytes)
{
    return now<K>(b, first, count, host, bytes, "sfl_batch_friction");
}
int sfl_batch_friction_start(sfl_batch *b, int every, int first, int count, int capacity)
{
    return start<K>(b, every, first, count, capacity, "sfl_batch_friction_start");
}
int sfl_batch_friction_stop(sfl_batch *b) { return stop<K>(b, "sfl_batch_friction_stop"); }
int sfl_batch_friction_info(sfl_batch *b, int *samples, int *capacity, int64_t *steps, int *bodies)
{
    return info<K>(b, samples, capacity, steps, bodies, "sfl_batch_friction_info");
}
int sfl_batch_friction_read(sfl_batch *b, int first_sample, int samples, struct sfl_body_friction *host, size_t bytes)
{
    return read<K>(b, first_sample, samples, host, bytes, "sfl_batch_friction_read");
}

int sfl_friction(sfl_context *ctx, struct sfl_body_friction *host, size_t bytes) { return now<K>(ctx, 0, 1, host, bytes, "sfl_friction"); }
int sfl_friction_start(sfl_context *ctx, int every, int capacity) { return start<K>(ctx, every, 0, 1, capacity, "sfl_friction_start"); }
int sfl_friction_stop(sfl_context *ctx) { return stop<K>(ctx, "sfl_friction_stop"); }
int sfl_friction_info(sfl_context *ctx, int *samples, int *capacity, int64_t *steps, int *bodies)
{
    return info<K>(ctx, samples, capacity, steps, bodies, "sfl_friction_info");
}
int sfl_friction_read(sfl_context *ctx, int first_sample, int samples, struct sfl_body_friction *host, size_t bytes)
{
    return read<K>(ctx, first_sample, samples, host, bytes, "sfl_friction_read");
}

}  // extern "C"
