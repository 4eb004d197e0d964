// history.cpp -- histories (include/sfl.h "HISTORIES"; sfl_batch_history_* of a batch of either kind, sfl_history_* of a
// whole-domain context): the flow statistics of every k-th step, sampled on the stream between the step launches and
// read out afterwards.  Host C++ only; a batch's sample is ONE launch of history.hip (history_kernels.h), a context's
// the streaming passes of flow_stats.hip and update_norm.hip pointed at the record.
//
// The step calls live in units that the host test harnesses link without this one, so they do not call into it: the
// history is plain data on the two structs (context.h History; freed by the destroy paths, its room checked and its cut
// points found by the step calls themselves through history_admit and history_run), and the sample is reached through
// their `history_step` pointer, set here while a history is on and null otherwise -- then a step call launches exactly
// what it launched before there were histories.
#include "batch_state.h"
#include "history_kernels.h"
#include "until_kernels.h"

using namespace sfl::host;

static_assert(sizeof(struct sfl_history_record) == 64 && offsetof(struct sfl_history_record, what) == 12 &&
                  offsetof(struct sfl_history_record, dye_sum) == 16 && offsetof(struct sfl_history_record, update_norm) == 40 &&
                  offsetof(struct sfl_history_record, iterations) == 44 && offsetof(struct sfl_history_record, step) == 48 &&
                  offsetof(struct sfl_history_record, dt) == 56 && offsetof(struct sfl_history_record, dx) == 60,
              "sfl_history_record: 64 bytes, offsets 0 4 8 12 16 40 44 48 56 60");
static_assert(offsetof(struct sfl_history_record, dye_sum) == offsetof(sfl::FlowStatsRecord, dye_sum) && sizeof(sfl::FlowStatsRecord) == 40,
              "the first 40 bytes of a record are what the flow statistics' passes write");

namespace {

constexpr size_t kRecord = sizeof(struct sfl_history_record);

struct Holder {
    History *h;
    hipStream_t stream;
    int device, members;
};
Holder holder_of(sfl_context *c) { return Holder{&c->history, c->stream, c->device, 1}; }
Holder holder_of(sfl_batch *b) { return Holder{&b->history, b->stream, b->device, b->batch}; }

int check_handle(sfl_context *c, const char *call)
{
    if (!c) return fail(SFL_ERR_INVALID, "%s: ctx is NULL", call);
    if (c->nranks != 1)   // (a slab's figures would need a reduction over the ranks)
        return fail(SFL_ERR_STATE, "%s: whole-domain contexts only (slab %d/%d)", call, c->rank, c->nranks);
    return SFL_OK;
}
int check_handle(sfl_batch *b, const char *call)
{
    if (!b) return fail(SFL_ERR_INVALID, "%s: batch is NULL", call);
    return SFL_OK;
}

// a sample's divergence and update norm are those of a grid without solid cells (include/sfl.h "SOLIDS"): a batch that has
// solids set starts no history (a running one is left as it is)
int check_solids(sfl_context *, const char *) { return SFL_OK; }
int check_solids(sfl_batch *b, const char *call)
{
    if (b->solids.set)
        return fail(SFL_ERR_STATE, "%s: the batch has solid cells set (sfl_batch_set_solids) and a history's samples do not know them: "
                    "no history started; clear the solids first (sfl_batch_set_solids(b, NULL, 0))", call);
    if (b->openings.set)   // (... nor those of a grid with openings: include/sfl.h "OPENINGS")
        return fail(SFL_ERR_STATE, "%s: the batch has openings set (sfl_batch_set_openings) and a history's samples do not know them: "
                    "no history started; clear the openings first (sfl_batch_set_openings(b, NULL, 0, NULL, 0))", call);
    return SFL_OK;
}

struct sfl_history_record *slot(const History &h, int sample) { return static_cast<struct sfl_history_record *>(h.d_records) + (size_t)sample * h.count; }

// counts `steps` steps (one launch: history_run saw to it that no sample falls inside them); the sample that is due now, or -1
int count_steps(History &h, int steps)
{
    h.steps += steps;
    if (h.steps % h.every != 0) return -1;
    return (int)(h.steps / h.every) - 1;   // < capacity: history_admit has let the call through
}

int step_batch(sfl_batch *b, int steps, const sfl::BatchMember *members, bool until, const sfl::SmallStep &step)
{
    History &h = b->history;
    const int sample = count_steps(h, steps);
    if (sample < 0) return SFL_OK;
    sfl::HistorySample a{};
    a.vel = b->vel;
    a.dye = b->col;
    a.p = b->p;
    a.d = b->div;
    a.dim_x = b->dim_x;
    a.dim_y = b->dim_y;
    a.first = h.first;
    a.count = h.count;
    a.batch = b->batch;
    a.step = h.steps;
    a.dt = step.dt;
    a.dx = step.prm.dx;
    a.two_dx_inv = step.two_dx_inv;
    a.iters = step.iters;
    a.members = members;
    a.counts = until ? b->d_counts : nullptr;
    a.out = slot(h, sample);
    HIP_TRY(sfl::launch_history_sample(b->stream, a));
    h.written = sample + 1;
    return SFL_OK;
}

int step_context(sfl_context *c, float dt, float dx, int iters)
{
    History &h = c->history;
    const int sample = count_steps(h, 1);
    if (sample < 0) return SFL_OK;
    SFL_TRY(ensure_field(c, SFL_FIELD_VELOCITY));
    SFL_TRY(ensure_field(c, SFL_FIELD_COLOR));
    SFL_TRY(ensure_field(c, SFL_FIELD_DIVERGENCE));
    SFL_TRY(ensure_field(c, SFL_FIELD_PRESSURE));
    SFL_TRY(use_device(c));
    struct sfl_history_record *rec = slot(h, sample);
    const float two_dx_inv = 1.0f / (2.0f * dx);  // finitediff.cpp:36
    HIP_TRY(sfl::launch_flow_stats(c->stream, reinterpret_cast<sfl::FlowStatsRecord *>(rec), SFL_STATS_VELOCITY | SFL_STATS_DYE, c->vel, c->col,
                                   c->dim_x, c->gdim_y, 1, two_dx_inv, nullptr));
    // (solid cells set: the divergence and the norm by their rule, as sfl_flow_stats and sfl_residual report them)
    if (c->solids.max_div) SFL_TRY(c->solids.max_div(c, two_dx_inv, &reinterpret_cast<sfl::FlowStatsRecord *>(rec)->max_abs_div));
    if (c->solids.norm)
        SFL_TRY(c->solids.norm(c, dx, reinterpret_cast<unsigned *>(&rec->update_norm)));
    else
        HIP_TRY(sfl::launch_update_norm(c->stream, reinterpret_cast<unsigned *>(&rec->update_norm), c->p, c->div, c->geom, c->g0, c->g1, dx));
    h.host_words[(size_t)sample] = History::HostWords{iters, h.steps, dt, dx};
    h.written = sample + 1;
    return SFL_OK;
}

// a context's passes know nothing of the step: the host keeps those words (context.h History::HostWords)
bool merges_host_words(sfl_context *) { return true; }
bool merges_host_words(sfl_batch *) { return false; }

void set_hook(sfl_context *c) { c->history_step = c->history.on ? step_context : nullptr; }
void set_hook(sfl_batch *b) { b->history_step = b->history.on ? step_batch : nullptr; }

template <class H>
int start(H *x, int every, int first, int count, int capacity, const char *call)
{
    if (every < 1) return fail(SFL_ERR_INVALID, "%s: every must be >= 1 (got %d)", call, every);
    if (capacity < 1) return fail(SFL_ERR_INVALID, "%s: capacity must be >= 1 (got %d)", call, capacity);
    if (count < 1) return fail(SFL_ERR_INVALID, "%s: count must be >= 1 (got %d)", call, count);
    const size_t sample_bytes = (size_t)count * kRecord;   // < 2^37
    if ((size_t)capacity > SIZE_MAX / sample_bytes)
        return fail(SFL_ERR_INVALID, "%s: capacity %d samples of %zu bytes each exceed the address space", call, capacity, sample_bytes);
    SFL_TRY(check_handle(x, call));
    const Holder o = holder_of(x);
    if (first < 0 || (int64_t)first + count > o.members)
        return fail(SFL_ERR_INVALID, "%s: members [%d, %d + %d) are not inside the batch's [0, %d)", call, first, first, count, o.members);
    SFL_TRY(check_solids(x, call));
    HIP_TRY(hipSetDevice(o.device));
    History &h = *o.h;
    // (samples of the history that ends here may still be in flight: they are ahead of the new ones on the stream)
    const size_t bytes = (size_t)capacity * sample_bytes;
    void *keep = h.d_records;
    size_t keep_bytes = h.d_bytes;
    h = History{};   // no history unless the samples are there
    h.d_records = keep;
    h.d_bytes = keep_bytes;
    set_hook(x);
    if (keep && bytes > keep_bytes) {   // a sample may still write the old records: drain on growth only
        HIP_TRY(hipStreamSynchronize(o.stream));
        (void)hipFree(keep);
        h.d_records = keep = nullptr;
        h.d_bytes = keep_bytes = 0;
    }
    if (!keep) {
        const hipError_t e = hipMalloc(&keep, bytes);
        if (e != hipSuccess) {
            (void)hipGetLastError();   // (so that the next launch's check does not report this failure again)
            return fail(e == hipErrorOutOfMemory ? SFL_ERR_NOMEM : SFL_ERR_HIP, "%s: hipMalloc of %zu bytes of samples failed: %s", call, bytes,
                        hipGetErrorString(e));
        }
        keep_bytes = bytes;
    }
    h.d_records = keep;
    h.d_bytes = keep_bytes;
    h.on = true;
    h.every = every;
    h.first = first;
    h.count = count;
    h.capacity = capacity;
    if (merges_host_words(x)) h.host_words.assign((size_t)capacity, History::HostWords{});
    set_hook(x);
    return SFL_OK;
}

template <class H>
int stop(H *x, const char *call)
{
    SFL_TRY(check_handle(x, call));
    const Holder o = holder_of(x);
    History &h = *o.h;
    void *records = h.d_records;
    h = History{};
    set_hook(x);
    if (!records) return SFL_OK;
    HIP_TRY(hipSetDevice(o.device));
    HIP_TRY(hipStreamSynchronize(o.stream));   // a sample may still write the records
    (void)hipFree(records);
    return SFL_OK;
}

template <class H>
int info(H *x, int *samples, int *capacity, int64_t *steps, const char *call)
{
    SFL_TRY(check_handle(x, call));
    const History &h = *holder_of(x).h;
    if (samples) *samples = h.written;
    if (capacity) *capacity = h.capacity;
    if (steps) *steps = h.steps;
    return SFL_OK;
}

template <class H>
int read(H *x, int first_sample, int samples, int first, int count, struct sfl_history_record *host, size_t bytes, const char *call)
{
    if (first_sample < 0 || samples < 0)
        return fail(SFL_ERR_INVALID, "%s: samples [%d, %d + %d): first_sample and samples must be >= 0", call, first_sample, first_sample, samples);
    if (count < 1) return fail(SFL_ERR_INVALID, "%s: count must be >= 1 (got %d)", call, count);
    const size_t want = (size_t)samples * (size_t)count * kRecord;   // < 2^31 * 2^31 * 2^6
    if (bytes != want)
        return fail(SFL_ERR_INVALID, "%s: %d samples of %d records of 64 bytes are %zu bytes, got %zu", call, samples, count, want, bytes);
    SFL_TRY(check_handle(x, call));
    const Holder o = holder_of(x);
    const History &h = *o.h;
    if (!h.on) return fail(SFL_ERR_STATE, "%s: no history to read: call sfl_history_start (sfl_batch_history_start) first", call);
    if ((int64_t)first_sample + samples > h.written)
        return fail(SFL_ERR_INVALID, "%s: samples [%d, %d + %d) are not inside the %d samples written so far, [0, %d)", call, first_sample,
                    first_sample, samples, h.written, h.written);
    if (first < h.first || (int64_t)first + count > (int64_t)h.first + h.count)
        return fail(SFL_ERR_INVALID, "%s: members [%d, %d + %d) are not inside the recorded [%d, %d + %d)", call, first, first, count, h.first,
                    h.first, h.count);
    if (samples == 0) return SFL_OK;
    if (!host) return fail(SFL_ERR_INVALID, "%s: host is NULL", call);
    HIP_TRY(hipSetDevice(o.device));
    const struct sfl_history_record *dev = slot(h, first_sample) + (first - h.first);
    if (count == h.count) {   // whole samples: one copy
        HIP_TRY(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, o.stream));
    } else {
        for (int s = 0; s < samples; ++s)
            HIP_TRY(hipMemcpyAsync(host + (size_t)s * count, dev + (size_t)s * h.count, (size_t)count * kRecord, hipMemcpyDeviceToHost, o.stream));
    }
    HIP_TRY(hipStreamSynchronize(o.stream));
    for (int s = 0; s < samples && !h.host_words.empty(); ++s) {   // a context: what the host knows of the sample
        const History::HostWords &w = h.host_words[(size_t)(first_sample + s)];
        host[s].what = SFL_STATS_VELOCITY | SFL_STATS_DYE;
        host[s].iterations = w.iterations;
        host[s].step = w.step;
        host[s].dt = w.dt;
        host[s].dx = w.dx;
    }
    return SFL_OK;
}

}  // namespace

extern "C" {

int sfl_batch_history_start(sfl_batch *b, int every, int first, int count, int capacity)
{
    return start(b, every, first, count, capacity, "sfl_batch_history_start");
}
int sfl_batch_history_stop(sfl_batch *b) { return stop(b, "sfl_batch_history_stop"); }
int sfl_batch_history_info(sfl_batch *b, int *samples, int *capacity, int64_t *steps)
{
    return info(b, samples, capacity, steps, "sfl_batch_history_info");
}
int sfl_batch_history_read(sfl_batch *b, int first_sample, int samples, int first, int count, struct sfl_history_record *host, size_t bytes)
{
    return read(b, first_sample, samples, first, count, host, bytes, "sfl_batch_history_read");
}

int sfl_history_start(sfl_context *ctx, int every, int capacity) { return start(ctx, every, 0, 1, capacity, "sfl_history_start"); }
int sfl_history_stop(sfl_context *ctx) { return stop(ctx, "sfl_history_stop"); }
int sfl_history_info(sfl_context *ctx, int *samples, int *capacity, int64_t *steps)
{
    return info(ctx, samples, capacity, steps, "sfl_history_info");
}
int sfl_history_read(sfl_context *ctx, int first_sample, int samples, struct sfl_history_record *host, size_t bytes)
{
    return read(ctx, first_sample, samples, 0, 1, host, bytes, "sfl_history_read");
}

}  // extern "C"
