// loads_driver.cpp -- TEST HARNESS (tests/cpp, `make -f loads.mk`; tests/test_loads.py): the HOST side of the loads
// (csrc/loads.cpp) and of its hooks in the step calls (csrc/batch.cpp, csrc/slab_step.cpp), run on a box without a GPU: the
// host units over the runtime that lives on the host (fake_hip.cpp) and kernels that do nothing (launch_stubs_ok.cpp).  The
// launchers of the batches, of the solids, of the histories and of the loads are stubs of THIS file that keep ONE log in the
// order of the calls, which is the order of the stream.  What is checked: the admission order -- a call's own argument checks,
// then the state refusals, each with its message, then (and only then) anything staged or launched; loads_admit refusing a
// call whole; steps counted across calls in both branches of run_steps and in sfl_step / sfl_step_n, the fused boundaries
// kept; samples zero-filled without solids; what the samplers are handed with solids; sfl_batch_set_bodies refused while
// recording; with the recorder off the launch log of a step call identical to one made before the recorder was started;
// destroy leaves no allocation.  Exit status 0 and "0 failed checks".
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../esp32-fluid-simulation_amd/csrc/batch_state.h"
#include "../../esp32-fluid-simulation_amd/csrc/history_kernels.h"
#include "../../esp32-fluid-simulation_amd/csrc/load_kernels.h"
#include "../../esp32-fluid-simulation_amd/csrc/solid_kernels.h"
#include "../../esp32-fluid-simulation_amd/csrc/until_kernels.h"
#include "../../esp32-fluid-simulation_amd/csrc/view_kernels.h"
#include "../../include/sfl.h"

extern "C" long fake_hip_live_allocations();

static int failures = 0;
#define CHECK(cond, ...)                                          \
    do {                                                          \
        if (!(cond)) {                                            \
            if (failures++ < 30) {                                \
                fprintf(stderr, "CHECK failed: %s -- ", #cond);   \
                fprintf(stderr, __VA_ARGS__);                     \
                fprintf(stderr, "\n");                            \
            }                                                     \
        }                                                         \
    } while (0)

// ---- the one log ---------------------------------------------------------------------------------------------------------
// 's' 'e' 'u' a batch's plain step (uniform, each, until), 'p' its replay (n: the steps), 'S' 'E' its step by the solids'
// rule; 'a' a context's velocity advection, 'A' its fused advection + divergence, 'M' a step seam, 'D' 'K' 'G' its masked
// divergence, solve launch and gradient; 'f' the statistics' pass, 'H' a batch history's sample; 'L' a batch's loads sample,
// 'C' a context's
struct Event {
    char kind;
    int n;
    sfl::BatchLoadSample batch;
    sfl::ContextLoadSample context;
};
static std::vector<Event> events;
static hipError_t note(char kind, int n = 0)
{
    events.push_back({kind, n, {}, {}});
    return hipSuccess;
}

namespace sfl {
bool small_grid_fits(int dim_x, int dim_y)   // (the real rule of small_grid.hip; launch_stubs_ok.cpp's answer is "no")
{
    return dim_x >= 2 && dim_y >= 2 && (long long)dim_x * dim_y <= kSmallGridMaxCells &&
           (long long)dim_y * ((dim_x + 1) / 2) <= kSmallGridMaxCells / 2;
}
hipError_t launch_advect_vec2f(hipStream_t, float *, const float *, const float *, Slab, int, int, int, int, float, bool, int *, const Slab *, int, int, int) { return note('a'); }
hipError_t launch_advect_divergence_tiled(hipStream_t, float *, float *, const float *, Slab, float, bool, float) { return note('A'); }
hipError_t launch_step_seam_tiled(hipStream_t, uint32_t *, const uint32_t *, float *, float *, const float *, const float *, Slab, float, float) { return note('M'); }
hipError_t launch_small_solve_warm(hipStream_t, float *, const float *, int, int, int, SorParams) { return hipSuccess; }
hipError_t launch_small_solve_until(hipStream_t, float *, const float *, int, int, int, SorParams, float, int, unsigned *result)
{
    result[0] = result[1] = 0;
    return hipSuccess;
}
hipError_t launch_update_norm(hipStream_t, unsigned *worst, const float *, const float *, Slab, int, int, float)
{
    *worst = 0;
    return hipSuccess;
}
hipError_t launch_flow_stats(hipStream_t, FlowStatsRecord *out, int what, const float *, const uint32_t *, int, int, int members, float, const float *)
{
    memset(out, 0, sizeof(FlowStatsRecord) * (size_t)members);
    return note('f', what);
}
hipError_t launch_view_scalar(hipStream_t, float *, const ViewFields &, int, float) { return hipSuccess; }
hipError_t launch_view_texels(hipStream_t, uint32_t *, const ViewFields &, const ViewParams &) { return hipSuccess; }
hipError_t launch_view_render(hipStream_t, uint16_t *, const ViewFields &, const ViewParams &, int, bool) { return hipSuccess; }
hipError_t launch_solid_divergence(hipStream_t, float *, float *, const uint8_t *, int, int, float, bool) { return note('D'); }
hipError_t launch_solid_gradient(hipStream_t, float *, const float *, const uint8_t *, int, int, float) { return note('G'); }
hipError_t launch_solid_sor(hipStream_t, float *, const float *, const float *, const uint8_t *, int, int, int k, SorParams) { return note('K', k); }
hipError_t launch_solid_update_norm(hipStream_t, unsigned *worst, const float *, const float *, const uint8_t *, int, int, float)
{
    *worst = 0;
    return hipSuccess;
}
hipError_t launch_solid_max_divergence(hipStream_t, unsigned *worst, const float *, const uint8_t *, int, int, float)
{
    *worst = 0;
    return hipSuccess;
}
hipError_t launch_batch_step(hipStream_t, const BatchStep &, int) { return note('s'); }
hipError_t launch_batch_step_each(hipStream_t, const BatchStep &, int, const BatchMember *, float *) { return note('e'); }
hipError_t launch_batch_step_until(hipStream_t, const BatchStep &, int, const BatchMember *, const BatchStop *, float *, int *, bool) { return note('u'); }
hipError_t launch_batch_large_step(hipStream_t, const BatchStep &, int) { return note('s'); }
hipError_t launch_batch_large_step_each(hipStream_t, const BatchStep &, int, const BatchMember *, float *) { return note('e'); }
hipError_t launch_batch_large_step_until(hipStream_t, const BatchStep &, int, const BatchMember *, const BatchStop *, float *, int *, bool) { return note('u'); }
hipError_t launch_batch_play(hipStream_t, const BatchPlay &a, int, const BatchMember *, float *) { return note('p', a.steps); }
hipError_t launch_batch_solve(hipStream_t, float *, const float *, int, int, int, int, SorParams) { return hipSuccess; }
hipError_t launch_batch_solve_each(hipStream_t, float *, const float *, int, int, int, const BatchMember *, float *) { return hipSuccess; }
hipError_t launch_batch_solve_until(hipStream_t, float *, const float *, int, int, int, const BatchMember *, const BatchStop *, float *, int *) { return hipSuccess; }
hipError_t launch_batch_large_solve(hipStream_t, float *, const float *, int, int, int, int, SorParams) { return hipSuccess; }
hipError_t launch_batch_large_solve_each(hipStream_t, float *, const float *, int, int, int, const BatchMember *, float *) { return hipSuccess; }
hipError_t launch_batch_large_solve_until(hipStream_t, float *, const float *, int, int, int, const BatchMember *, const BatchStop *, float *, int *) { return hipSuccess; }
hipError_t launch_batch_solid_step(hipStream_t, const BatchStep &, const BatchSolids &, int) { return note('S'); }
hipError_t launch_batch_solid_step_each(hipStream_t, const BatchStep &, const BatchSolids &, int, const BatchMember *, float *) { return note('E'); }
hipError_t launch_batch_solid_solve(hipStream_t, float *, const float *, const BatchSolids &, int, int, int, int, SorParams) { return hipSuccess; }
hipError_t launch_batch_solid_solve_each(hipStream_t, float *, const float *, const BatchSolids &, int, int, int, const BatchMember *, float *) { return hipSuccess; }
hipError_t launch_solid_velocity_stats(hipStream_t, FlowStatsRecord *, const float *, const BatchSolids &, int, int, int, float, const float *) { return hipSuccess; }
hipError_t launch_batch_render(hipStream_t, uint16_t *, const uint32_t *, int, int, int, int, bool) { return hipSuccess; }
hipError_t launch_history_sample(hipStream_t, const HistorySample &a, int)
{
    for (int k = 0; k < a.count; ++k) memset(&a.out[k], 0, sizeof a.out[k]);
    return note('H');
}
// the samplers: the records they are to write get a mark, so that a sample that was launched differs from a zeroed one
hipError_t launch_batch_loads(hipStream_t, const BatchLoadSample &a)
{
    memset(a.out, 0x5a, sizeof(struct sfl_body_load) * (size_t)a.count * a.bodies);
    events.push_back({'L', a.count, a, {}});
    return hipSuccess;
}
hipError_t launch_context_loads(hipStream_t, const ContextLoadSample &a)
{
    memset(a.out, 0x5a, sizeof(struct sfl_body_load) * (size_t)a.bodies);
    events.push_back({'C', a.bodies, {}, a});
    return hipSuccess;
}
}  // namespace sfl

static const float DT = 0.03f, DX = 0.7f, OMEGA = 1.9f;
static bool says(const char *word) { return strstr(sfl_last_error(), word) != nullptr; }
static std::string kinds()
{
    std::string s;
    for (const Event &e : events) s += e.kind;
    return s;
}
static bool all_bytes(const void *p, size_t n, int v)
{
    for (size_t k = 0; k < n; ++k)
        if (static_cast<const uint8_t *>(p)[k] != (uint8_t)v) return false;
    return true;
}

static const int B = 3, X = 4, Y = 3, CELLS = X * Y;
static const uint8_t MASK[CELLS] = {0, 1, 0, 0, 0, 0, 7, 0, 0, 0, 0, 1};
static const size_t REC = sizeof(struct sfl_body_load);

template <class H>
static bool info_is(H *x, int (*info)(H *, int *, int *, int64_t *, int *), int samples, int capacity, int64_t steps, int bodies)
{
    int s = -1, c = -1, n = -1;
    int64_t t = -1;
    const bool ok = info(x, &s, &c, &t, &n) == SFL_OK && s == samples && c == capacity && t == steps && n == bodies;
    if (!ok) fprintf(stderr, "  info: %d samples, capacity %d, %lld steps, %d bodies\n", s, c, (long long)t, n);
    return ok;
}

static void refusals_without_handles()
{
    uint8_t lab[CELLS] = {};
    struct sfl_body_load rec[4];
    int w = 5;
    CHECK(sfl_batch_set_bodies(nullptr, lab, 2, 1) == SFL_ERR_INVALID && says("sfl_batch_set_bodies: per_member must be 0 or 1 (got 2)"), "%s", sfl_last_error());
    CHECK(sfl_batch_set_bodies(nullptr, lab, 0, 0) == SFL_ERR_INVALID && says("bodies must be 1..16 (got 0)"), "%s", sfl_last_error());
    CHECK(sfl_batch_set_bodies(nullptr, lab, 0, 17) == SFL_ERR_INVALID && says("bodies must be 1..16 (got 17)"), "%s", sfl_last_error());
    CHECK(sfl_batch_set_bodies(nullptr, lab, 0, 1) == SFL_ERR_INVALID && says("sfl_batch_set_bodies: batch is NULL"), "%s", sfl_last_error());
    CHECK(sfl_batch_bodies_info(nullptr, &w, &w, &w) == SFL_ERR_INVALID && says("sfl_batch_bodies_info: batch is NULL") && w == 5, "%s", sfl_last_error());
    CHECK(sfl_batch_bodies_download(nullptr, 0, 1, lab, CELLS) == SFL_ERR_INVALID && says("sfl_batch_bodies_download: batch is NULL"), "%s", sfl_last_error());
    CHECK(sfl_batch_loads(nullptr, 0, 1, rec, REC) == SFL_ERR_INVALID && says("sfl_batch_loads: batch is NULL"), "%s", sfl_last_error());
    CHECK(sfl_batch_loads_start(nullptr, 0, 0, 1, 1) == SFL_ERR_INVALID && says("sfl_batch_loads_start: every must be >= 1 (got 0)"), "%s", sfl_last_error());
    CHECK(sfl_batch_loads_start(nullptr, 1, 0, 1, 0) == SFL_ERR_INVALID && says("capacity must be >= 1 (got 0)"), "%s", sfl_last_error());
    CHECK(sfl_batch_loads_start(nullptr, 1, 0, 0, 1) == SFL_ERR_INVALID && says("count must be >= 1 (got 0)"), "%s", sfl_last_error());
    CHECK(sfl_batch_loads_start(nullptr, 1, 0, 1, 1) == SFL_ERR_INVALID && says("sfl_batch_loads_start: batch is NULL"), "%s", sfl_last_error());
    CHECK(sfl_batch_loads_stop(nullptr) == SFL_ERR_INVALID && says("sfl_batch_loads_stop: batch is NULL"), "%s", sfl_last_error());
    CHECK(sfl_batch_loads_info(nullptr, &w, &w, nullptr, &w) == SFL_ERR_INVALID && says("sfl_batch_loads_info: batch is NULL") && w == 5, "%s", sfl_last_error());
    CHECK(sfl_batch_loads_read(nullptr, -1, 0, rec, 0) == SFL_ERR_INVALID && says("first_sample and samples must be >= 0"), "%s", sfl_last_error());
    CHECK(sfl_batch_loads_read(nullptr, 0, 0, rec, 0) == SFL_ERR_INVALID && says("sfl_batch_loads_read: batch is NULL"), "%s", sfl_last_error());
    CHECK(sfl_set_bodies(nullptr, lab, 17) == SFL_ERR_INVALID && says("sfl_set_bodies: bodies must be 1..16"), "%s", sfl_last_error());
    CHECK(sfl_set_bodies(nullptr, lab, 1) == SFL_ERR_INVALID && says("sfl_set_bodies: ctx is NULL"), "%s", sfl_last_error());
    CHECK(sfl_bodies_info(nullptr, &w, &w) == SFL_ERR_INVALID && says("sfl_bodies_info: ctx is NULL"), "%s", sfl_last_error());
    CHECK(sfl_bodies_download(nullptr, lab, CELLS) == SFL_ERR_INVALID && says("sfl_bodies_download: ctx is NULL"), "%s", sfl_last_error());
    CHECK(sfl_loads(nullptr, rec, REC) == SFL_ERR_INVALID && says("sfl_loads: ctx is NULL"), "%s", sfl_last_error());
    CHECK(sfl_loads_start(nullptr, 0, 1) == SFL_ERR_INVALID && says("sfl_loads_start: every must be >= 1"), "%s", sfl_last_error());
    CHECK(sfl_loads_start(nullptr, 1, 1) == SFL_ERR_INVALID && says("sfl_loads_start: ctx is NULL"), "%s", sfl_last_error());
    CHECK(sfl_loads_stop(nullptr) == SFL_ERR_INVALID && says("sfl_loads_stop: ctx is NULL"), "%s", sfl_last_error());
    CHECK(sfl_loads_info(nullptr, &w, &w, nullptr, &w) == SFL_ERR_INVALID && says("sfl_loads_info: ctx is NULL"), "%s", sfl_last_error());
    CHECK(sfl_loads_read(nullptr, 0, 0, rec, 0) == SFL_ERR_INVALID && says("sfl_loads_read: ctx is NULL"), "%s", sfl_last_error());
    CHECK(events.empty(), "a refused call launches nothing");
}

static void batches()
{
    sfl_batch *b = nullptr, *large = nullptr;
    CHECK(sfl_batch_create(&b, 0, X, Y, B) == SFL_OK && sfl_batch_create_large(&large, 0, X, Y, B) == SFL_OK && b && large, "create: %s", sfl_last_error());
    if (!b || !large) return;
    sfl_member_params prm[B];
    for (int m = 0; m < B; ++m) prm[m] = {DT * (m + 1), DX, OMEGA, 3 + m};
    struct sfl_body_load rec[B * 3 * 4];
    const auto baseline = [&] { return sfl_batch_step_n(b, 2, DT, DX, 4, OMEGA) == SFL_OK && sfl_batch_step_n_each(b, 1, prm) == SFL_OK; };
    // ---- before there is a recorder: the log to compare with; no solids: zero records without a launch
    events.clear();
    CHECK(baseline() && kinds() == "sse" && b->loads_step == nullptr, "baseline: %s", kinds().c_str());
    const std::string log0 = kinds();
    events.clear();
    int n = -1, lab = -1, per = -1;
    CHECK(sfl_batch_bodies_info(b, &n, &lab, &per) == SFL_OK && n == 1 && lab == 0 && per == 0, "bodies at first: %d %d %d", n, lab, per);
    memset(rec, 0xff, sizeof rec);
    CHECK(sfl_batch_loads(b, 0, B, rec, B * REC) == SFL_OK && all_bytes(rec, B * REC, 0) && events.empty() && b->loads.d_records == nullptr,
          "no solids: zeros, no launch, no allocation: %s", sfl_last_error());
    CHECK(sfl_batch_loads(b, 1, 3, rec, 3 * REC) == SFL_ERR_INVALID && says("not inside the batch's [0, 3)"), "range: %s", sfl_last_error());
    CHECK(sfl_batch_loads(b, 0, 2, rec, REC) == SFL_ERR_INVALID && says("2 members of 1 records of 48 bytes are 96 bytes, got 48"), "bytes: %s", sfl_last_error());
    CHECK(sfl_batch_loads(b, 0, 2, nullptr, 2 * REC) == SFL_ERR_INVALID && says("host is NULL"), "host: %s", sfl_last_error());
    CHECK(sfl_batch_loads_read(b, 0, 0, rec, 0) == SFL_ERR_STATE && says("no loads recorder to read"), "read without: %s", sfl_last_error());
    // ---- the recorder without solids: steps counted across calls, samples zero-filled, nothing launched for them
    CHECK(sfl_batch_loads_start(b, 2, 2, 2, 2) == SFL_ERR_INVALID && says("members [2, 2 + 2) are not inside the batch's [0, 3)") && !b->loads.on, "start: range: %s", sfl_last_error());
    CHECK(sfl_batch_loads_start(b, 2, 1, 2, 2) == SFL_OK && b->loads.on && b->loads_step && info_is(b, sfl_batch_loads_info, 0, 2, 0, 1), "start: %s", sfl_last_error());
    CHECK(b->loads.d_bytes == (B + 2 * 2) * REC, "the records: one sample of every member in front, then capacity x count: %zu", b->loads.d_bytes);
    void *buffer = b->loads.d_records;
    memset(buffer, 0xff, b->loads.d_bytes);
    events.clear();
    CHECK(sfl_batch_step_n(b, 3, DT, DX, 4, OMEGA) == SFL_OK && kinds() == "sss" && info_is(b, sfl_batch_loads_info, 1, 2, 3, 1), "3 steps: %s", kinds().c_str());
    CHECK(sfl_batch_step_n_each(b, 1, prm) == SFL_OK && kinds() == "ssse" && info_is(b, sfl_batch_loads_info, 2, 2, 4, 1), "... and one more, by the _each call: %s", kinds().c_str());
    CHECK(sfl_batch_loads_read(b, 0, 2, rec, 2 * 2 * REC) == SFL_OK && all_bytes(rec, 4 * REC, 0), "without solids a sample is zero records");
    CHECK(all_bytes(buffer, B * REC, 0xff), "... and the room of the synchronous call is not a sample's");
    CHECK(sfl_batch_loads_read(b, 1, 2, rec, 4 * REC) == SFL_ERR_INVALID && says("not inside the 2 samples written so far"), "read: range: %s", sfl_last_error());
    CHECK(sfl_batch_loads_read(b, 0, 2, rec, 3 * REC) == SFL_ERR_INVALID && says("2 samples of 2 records of 48 bytes (2 members of 1 bodies) are 192 bytes, got 144"), "read: bytes: %s", sfl_last_error());
    // ---- full: a step call is refused whole, its own argument checks first
    const int ms[2] = {0, 2}, cells[4] = {0, 0, 1, 0};
    const float vels[4] = {1, 0, 0, 1};
    CHECK(sfl_batch_queue_forces_at(b, 0, ms, cells, vels, 1) == SFL_OK, "a record to keep");
    events.clear();
    sfl::BatchMember *members_before = b->d_members;
    const int slot_before = b->member_slot;
    int pending = -1;
    CHECK(sfl_batch_step_n(b, 2, DT, DX, -1, OMEGA) == SFL_ERR_INVALID && says("iters must be >= 0"), "iters first: %s", sfl_last_error());
    CHECK(sfl_batch_step_n(b, 2, DT, DX, 4, OMEGA) == SFL_ERR_STATE && says("the loads recorder has room for 0 more samples (2 of 2 written) and 2 steps would complete 1") &&
              says("sfl_batch_loads_read"), "step_n while full: %s", sfl_last_error());
    CHECK(sfl_batch_step_n_each(b, 2, prm) == SFL_ERR_STATE && says("loads recorder") && sfl_batch_step_n_each(b, 2, nullptr) == SFL_ERR_INVALID, "step_n_each while full");
    sfl_member_stop stop[B] = {{-1.0f, 2}, {-1.0f, 2}, {-1.0f, 2}};
    CHECK(sfl_batch_step_n_until(b, 2, prm, stop) == SFL_ERR_STATE && says("loads recorder"), "step_n_until while full: %s", sfl_last_error());
    CHECK(events.empty() && b->d_members == members_before && b->member_slot == slot_before && info_is(b, sfl_batch_loads_info, 2, 2, 4, 1) &&
              sfl_batch_forces_pending(b, &pending, nullptr) == SFL_OK && pending == 1, "a refused call stages, launches and counts nothing");
    CHECK(sfl_batch_step_n(b, 1, DT, DX, 4, OMEGA) == SFL_OK && kinds() == "s" && info_is(b, sfl_batch_loads_info, 2, 2, 5, 1), "one step completes none: let through");
    // ---- set_bodies while recording: its own checks first, then the refusal
    uint8_t labels[B * CELLS];
    for (int k = 0; k < B * CELLS; ++k) labels[k] = (uint8_t)(k % 4);
    CHECK(sfl_batch_set_bodies(b, labels, 0, 2) == SFL_ERR_INVALID && says("label 3 of cell (3, 0) of member 0 exceeds bodies = 2"), "the first offending cell: %s", sfl_last_error());
    CHECK(sfl_batch_set_bodies(b, labels, 0, 3) == SFL_ERR_STATE && says("the loads recorder is on") && says("sfl_batch_loads_stop") && b->loads.d_labels == nullptr && b->loads.bodies == 1,
          "set_bodies while recording: %s", sfl_last_error());
    CHECK(sfl_batch_set_bodies(b, nullptr, 0, 1) == SFL_ERR_STATE, "... going back too");
    // ---- a restart keeps the buffer; with solids the sampler is launched behind the step that is due
    CHECK(sfl_batch_loads_start(b, 2, 1, 2, 2) == SFL_OK && b->loads.d_records == buffer && info_is(b, sfl_batch_loads_info, 0, 2, 0, 1), "restart: %s", sfl_last_error());
    CHECK(sfl_batch_set_solids(b, MASK, 0) == SFL_OK, "solids: %s", sfl_last_error());
    events.clear();
    CHECK(sfl_batch_step_n(b, 2, DT, DX, 4, OMEGA) == SFL_OK && kinds() == "SSL" && info_is(b, sfl_batch_loads_info, 1, 2, 2, 1), "with solids: %s", kinds().c_str());
    if (kinds() == "SSL") {
        const sfl::BatchLoadSample &a = events[2].batch;
        CHECK(a.p == b->p && a.codes == b->solids.d_codes && a.code_stride == 0 && a.labels == nullptr && a.dim_x == X && a.dim_y == Y && a.first == 1 && a.count == 2 &&
                  a.bodies == 1 && a.out == static_cast<struct sfl_body_load *>(buffer) + B, "what the sampler is handed");
    }
    CHECK(sfl_batch_step_n_each(b, 2, prm) == SFL_OK && kinds() == "SSLEEL" && events[5].batch.out == static_cast<struct sfl_body_load *>(buffer) + B + 2, "the second sample's slot: %s", kinds().c_str());
    CHECK(sfl_batch_loads_read(b, 0, 2, rec, 4 * REC) == SFL_OK && all_bytes(rec, 4 * REC, 0x5a), "the samples that were launched");
    // the synchronous call beside the recorder: the room in front
    events.clear();
    CHECK(sfl_batch_loads(b, 2, 1, rec, REC) == SFL_OK && kinds() == "L" && events[0].batch.first == 2 && events[0].batch.count == 1 && events[0].batch.out == buffer &&
              b->loads.d_records == buffer && all_bytes(rec, REC, 0x5a), "loads beside the recorder: %s", sfl_last_error());
    // ---- a timeline replayed in one launch: no cut, the samples inside are zeros
    CHECK(sfl_batch_set_solids(b, nullptr, 0) == SFL_OK && sfl_batch_forget_forces(b) == SFL_OK && sfl_batch_loads_start(b, 1, 0, B, 4) == SFL_OK, "every step, no solids: %s", sfl_last_error());
    buffer = b->loads.d_records;
    memset(buffer, 0xff, b->loads.d_bytes);
    CHECK(sfl_batch_queue_forces_at(b, 0, ms, cells, vels, 1) == SFL_OK && sfl_batch_queue_forces_at(b, 2, ms + 1, cells + 2, vels + 2, 1) == SFL_OK, "a timeline");
    events.clear();
    CHECK(sfl_batch_step_n(b, 4, DT, DX, 4, OMEGA) == SFL_OK && kinds() == "p" && events[0].n == 4 && info_is(b, sfl_batch_loads_info, 4, 4, 4, 1), "the replay is not cut: %s", kinds().c_str());
    CHECK(sfl_batch_loads_read(b, 0, 4, rec, 4 * B * REC) == SFL_OK && all_bytes(rec, 4 * B * REC, 0), "its samples are zeros");
    // ... and a history beside it cuts as it did, the loads' hook behind the history's
    CHECK(sfl_batch_loads_start(b, 2, 0, B, 4) == SFL_OK && sfl_batch_history_start(b, 2, 0, B, 4) == SFL_OK, "both: %s", sfl_last_error());
    CHECK(sfl_batch_queue_forces_at(b, 0, ms, cells, vels, 1) == SFL_OK && sfl_batch_queue_forces_at(b, 2, ms + 1, cells + 2, vels + 2, 1) == SFL_OK, "a timeline");
    events.clear();
    CHECK(sfl_batch_step_n(b, 4, DT, DX, 4, OMEGA) == SFL_OK && kinds() == "pHpH" && info_is(b, sfl_batch_loads_info, 2, 4, 4, 1), "with a history: %s", kinds().c_str());
    CHECK(sfl_batch_history_stop(b) == SFL_OK, "history off");
    // ---- stopped: the hook is gone, the buffer freed, the launch log the one from before the recorder
    CHECK(sfl_batch_loads_stop(b) == SFL_OK && b->loads_step == nullptr && !b->loads.on && b->loads.d_records == nullptr && info_is(b, sfl_batch_loads_info, 0, 0, 0, 1), "stop");
    CHECK(sfl_batch_loads_stop(b) == SFL_OK, "stop without a recorder");
    events.clear();
    CHECK(baseline() && kinds() == log0, "recorder off: the log of before (%s, %s)", kinds().c_str(), log0.c_str());
    // ---- labels: shared and per member, either before or after the mask; the sampler's strides
    uint8_t got[B * CELLS];
    CHECK(sfl_batch_set_bodies(b, labels, 0, 3) == SFL_OK && sfl_batch_bodies_info(b, &n, &lab, &per) == SFL_OK && n == 3 && lab == 1 && per == 0 &&
              b->loads.d_label_bytes == (size_t)CELLS, "labels, shared, before the mask: %s", sfl_last_error());
    CHECK(sfl_batch_bodies_download(b, 1, 2, got, 2 * CELLS) == SFL_OK && memcmp(got, labels, CELLS) == 0 && memcmp(got + CELLS, labels, CELLS) == 0, "download: shared labels repeated");
    CHECK(sfl_batch_loads(b, 0, B, rec, 3 * B * REC) == SFL_OK && all_bytes(rec, 3 * B * REC, 0), "labels but no solids: zeros");
    uint8_t each[B * CELLS] = {};
    memcpy(each + CELLS, MASK, CELLS);
    CHECK(sfl_batch_set_solids(b, each, 1) == SFL_OK, "masks per member");
    events.clear();
    CHECK(sfl_batch_loads(b, 0, B, rec, 3 * B * REC) == SFL_OK && kinds() == "L" && events[0].batch.bodies == 3 && events[0].batch.labels == b->loads.d_labels &&
              events[0].batch.label_stride == 0 && events[0].batch.code_stride == (size_t)CELLS && b->loads.d_bytes == 3 * B * REC, "shared labels, masks per member: %s", sfl_last_error());
    CHECK(sfl_batch_set_bodies(b, labels, 1, 3) == SFL_OK && sfl_batch_bodies_info(b, &n, &lab, &per) == SFL_OK && n == 3 && lab == 1 && per == 1 && sfl_batch_set_solids(b, MASK, 0) == SFL_OK,
          "labels per member, mask shared: %s", sfl_last_error());
    events.clear();
    CHECK(sfl_batch_loads(b, 1, 2, rec, 3 * 2 * REC) == SFL_OK && kinds() == "L" && events[0].batch.label_stride == (size_t)CELLS && events[0].batch.code_stride == 0 &&
              events[0].batch.first == 1, "the two strides are independent");
    CHECK(sfl_batch_bodies_download(b, 2, 1, got, CELLS) == SFL_OK && memcmp(got, labels + 2 * CELLS, CELLS) == 0, "download, per member");
    CHECK(sfl_batch_set_bodies(b, nullptr, 0, 9) == SFL_OK && sfl_batch_bodies_info(b, &n, &lab, &per) == SFL_OK && n == 1 && lab == 0 && per == 0 && b->loads.d_labels == nullptr,
          "labels NULL: every solid is body 1 again");
    CHECK(sfl_batch_bodies_download(b, 0, 1, got, CELLS) == SFL_OK && all_bytes(got, CELLS, 1), "... and the download says so");
    // ---- a large batch has no solids: zeros, and a recorder that zero-fills
    events.clear();
    CHECK(sfl_batch_loads(large, 0, B, rec, B * REC) == SFL_OK && all_bytes(rec, B * REC, 0) && sfl_batch_loads_start(large, 1, 0, B, 2) == SFL_OK &&
              sfl_batch_step_n(large, 2, DT, DX, 4, OMEGA) == SFL_OK && kinds() == "ss" && info_is(large, sfl_batch_loads_info, 2, 2, 2, 1), "large: %s (%s)", kinds().c_str(), sfl_last_error());
    // ---- destroy with labels set and a recorder on
    CHECK(sfl_batch_set_bodies(b, labels, 1, 3) == SFL_OK && sfl_batch_loads_start(b, 1, 0, B, 2) == SFL_OK, "labels and a recorder to destroy");
    CHECK(sfl_batch_destroy(b) == SFL_OK && sfl_batch_destroy(large) == SFL_OK, "destroy");
    events.clear();
}

static void contexts()
{
    const int CX = 8, CY = 6, CC = CX * CY;
    sfl_context *c = nullptr, *slab = nullptr;
    CHECK(sfl_create(&c, 0, CX, CY) == SFL_OK && sfl_create_slab(&slab, 0, CX, 2 * CY, 0, 2) == SFL_OK && c && slab, "create: %s", sfl_last_error());
    if (!c || !slab) return;
    uint8_t mask[CC] = {}, labels[CC] = {}, got[CC];
    mask[2 * CX + 3] = mask[2 * CX + 4] = 1;
    labels[2 * CX + 3] = 1, labels[2 * CX + 4] = 2;
    struct sfl_body_load rec[8];
    // ---- a slab: refused, the call's own checks first
    CHECK(sfl_set_bodies(slab, labels, 0) == SFL_ERR_INVALID && says("bodies must be"), "slab: bodies first: %s", sfl_last_error());
    CHECK(sfl_set_bodies(slab, labels, 2) == SFL_ERR_STATE && says("sfl_set_bodies: whole-domain contexts only (slab 0/2)"), "slab: %s", sfl_last_error());
    CHECK(sfl_loads(slab, rec, REC) == SFL_ERR_STATE && says("sfl_loads: whole-domain contexts only"), "slab: %s", sfl_last_error());
    CHECK(sfl_loads_start(slab, 0, 1) == SFL_ERR_INVALID && sfl_loads_start(slab, 1, 1) == SFL_ERR_STATE && says("sfl_loads_start: whole-domain contexts only") && !slab->loads.on &&
              slab->loads_step == nullptr, "slab: %s", sfl_last_error());
    CHECK(sfl_bodies_download(slab, got, CC) == SFL_ERR_STATE && sfl_loads_read(slab, 0, 0, rec, 0) == SFL_ERR_STATE, "slab: download and read");
    CHECK(sfl_loads_stop(slab) == SFL_OK && sfl_set_bodies(slab, nullptr, 1) == SFL_OK, "slab: stopping and un-labelling are let through");
    // ---- before there is a recorder; the fused boundaries of sfl_step_n on the tiled kernels
    CHECK(sfl_set_option(c, SFL_OPT_ADVECT_KERNEL, 2) == SFL_OK && sfl_set_option(c, SFL_OPT_SMALL_GRID, 0) == SFL_OK, "tiled, no one-launch step");
    const auto baseline = [&] { return sfl_step(c, DT, DX, 4, OMEGA) == SFL_OK && sfl_step_n(c, 3, DT, DX, 4, OMEGA) == SFL_OK; };
    events.clear();
    CHECK(baseline() && c->loads_step == nullptr, "baseline: %s", sfl_last_error());
    const std::string log0 = kinds();
    CHECK(log0 == "AAMM", "a step, then three with two seams: %s", log0.c_str());
    CHECK(sfl_loads(c, rec, REC) == SFL_OK && all_bytes(rec, REC, 0) && kinds() == log0 && c->loads.d_records == nullptr, "no solids: zeros, no launch");
    CHECK(sfl_loads(c, rec, 2 * REC) == SFL_ERR_INVALID && says("sfl_loads: the records of 1 bodies of 48 bytes each are 48 bytes, got 96") && !says("member"), "bytes: %s", sfl_last_error());
    // ---- the recorder without solids keeps the seams and zero-fills
    CHECK(sfl_loads_start(c, 2, 2) == SFL_OK && c->loads_step && c->loads.d_bytes == 3 * REC, "start: %s", sfl_last_error());
    memset(c->loads.d_records, 0xff, c->loads.d_bytes);
    events.clear();
    CHECK(baseline() && kinds() == log0 && info_is(c, sfl_loads_info, 2, 2, 4, 1), "recorder on, no solids: the same launches (%s)", kinds().c_str());
    CHECK(sfl_loads_read(c, 0, 2, rec, 2 * REC) == SFL_OK && all_bytes(rec, 2 * REC, 0), "two zero samples");
    events.clear();
    CHECK(sfl_step_n(c, 2, DT, DX, -1, OMEGA) == SFL_ERR_INVALID && says("iters must be >= 0"), "iters first: %s", sfl_last_error());
    CHECK(sfl_step_n(c, 2, DT, DX, 4, OMEGA) == SFL_ERR_STATE && says("the loads recorder has room for 0 more samples") && sfl_step_n(c, 1, DT, DX, 4, OMEGA) == SFL_OK &&
              sfl_step(c, DT, DX, 4, OMEGA) == SFL_ERR_STATE && kinds() == "A" && info_is(c, sfl_loads_info, 2, 2, 5, 1), "full: refused whole: %s (%s)", kinds().c_str(), sfl_last_error());
    // ---- labels and a mask: the sampler behind the history's passes, last
    CHECK(sfl_set_bodies(c, labels, 2) == SFL_ERR_STATE && says("the loads recorder is on"), "set_bodies while recording: %s", sfl_last_error());
    CHECK(sfl_loads_stop(c) == SFL_OK && c->loads_step == nullptr && c->loads.d_records == nullptr, "stop");
    labels[5] = 3;
    CHECK(sfl_set_bodies(c, labels, 2) == SFL_ERR_INVALID && says("sfl_set_bodies: label 3 of cell (5, 0) exceeds bodies = 2"), "the first offending cell: %s", sfl_last_error());
    labels[5] = 0;
    int n = -1, lab = -1;
    CHECK(sfl_set_bodies(c, labels, 2) == SFL_OK && sfl_bodies_info(c, &n, &lab) == SFL_OK && n == 2 && lab == 1 && sfl_bodies_download(c, got, CC) == SFL_OK && memcmp(got, labels, CC) == 0,
          "labels: %s", sfl_last_error());
    CHECK(sfl_set_solids(c, mask) == SFL_OK && sfl_loads_start(c, 2, 2) == SFL_OK && sfl_history_start(c, 1, 8) == SFL_OK && c->loads.d_bytes == (2 + 2 * 2) * REC, "mask, both recorders: %s", sfl_last_error());
    events.clear();
    CHECK(sfl_step_n(c, 2, DT, DX, 4, OMEGA) == SFL_OK && kinds() == "aDKGfaDKGfC" && info_is(c, sfl_loads_info, 1, 2, 2, 2), "with solids: %s", kinds().c_str());
    if (!events.empty() && events.back().kind == 'C') {
        const sfl::ContextLoadSample &a = events.back().context;
        CHECK(a.p == c->p && a.codes == c->solids.d_codes && a.labels == c->loads.d_labels && a.dim_x == CX && a.dim_y == CY && a.bodies == 2 &&
                  a.out == static_cast<struct sfl_body_load *>(c->loads.d_records) + 2, "what the sampler is handed");
    }
    events.clear();
    CHECK(sfl_loads(c, rec, 2 * REC) == SFL_OK && kinds() == "C" && events[0].context.out == c->loads.d_records && all_bytes(rec, 2 * REC, 0x5a), "loads beside the recorder");
    CHECK(sfl_loads_read(c, 0, 1, rec, 2 * REC) == SFL_OK && all_bytes(rec, 2 * REC, 0x5a), "the sample");
    CHECK(sfl_loads_read(c, 0, 1, rec, REC) == SFL_ERR_INVALID && says("1 samples of 2 records of 48 bytes (1 context of 2 bodies) are 96 bytes, got 48"), "read: bytes: %s", sfl_last_error());
    CHECK(sfl_bodies_download(c, got, CC - 1) == SFL_ERR_INVALID && says("sfl_bodies_download: the labels of 8 x 6 cells are 48 bytes, got 47") && !says("member"), "download: bytes: %s", sfl_last_error());
    // ---- recorder off: the log of a run without one
    CHECK(sfl_history_stop(c) == SFL_OK && sfl_set_solids(c, nullptr) == SFL_OK && sfl_loads_stop(c) == SFL_OK, "all off");
    events.clear();
    CHECK(baseline() && kinds() == log0, "recorder off: the log of before (%s)", kinds().c_str());
    CHECK(sfl_loads_start(c, 1, 2) == SFL_OK, "a recorder to destroy");
    CHECK(sfl_destroy(c) == SFL_OK && sfl_destroy(slab) == SFL_OK, "destroy");
    events.clear();
}

int main()
{
    refusals_without_handles();
    batches();
    contexts();
    const long left = fake_hip_live_allocations();
    printf("loads driver: %d failed checks, %ld allocations left\n", failures, left);
    return failures || left ? 1 : 0;
}
