// tracers_driver.cpp -- TEST HARNESS (tests/cpp, `make -f tracers.mk`; tests/test_tracers.py): the HOST side of the tracers
// (csrc/tracers.cpp) and of their hook in the step calls, run on a box without a GPU under AddressSanitizer + UBSan: the host
// units of contexts and batches over the runtime that lives on the host (fake_hip.cpp) and kernels that do nothing
// (launch_stubs_ok.cpp).  The launchers of csrc/tracer_kernels.h, the step launchers of the batches (csrc/batch.h) and the two
// kernels that end a step of a tiled context (kernels.h: the projection fused into the dye's advection, and the seam between
// two steps) are stubs of THIS file that keep ONE log in the order of the calls, which is the order of the stream.  What is
// checked: without a set, and with a set that does not follow, step_n, step_n_each, step_n_until, the replay of a timeline
// and a context's seams log what they always logged and no tracer launch; with a following set exactly one advance follows
// every step, on the velocity that step wrote, with that call's member table or dt, and neither a replay nor a seam hides a
// step; the trail's slots and counts; a call without room for its slots is refused whole; every refusal with its message;
// set, replace, remove and destroy with a live trail leave no allocation.  Exit status 0 and "0 failed checks" = all of it.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../esp32-fluid-simulation_amd/csrc/batch_state.h"
#include "../../esp32-fluid-simulation_amd/csrc/tracer_kernels.h"
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
struct Event {
    char kind;   // 's' 'e' 'u' a batch's step (uniform, each, until), 'p' its replay, 'P' a context's step ends with its projected
                 // velocity stored, 'M' a seam ends one step and begins the next, 'A' a tracer advance, 'Q' a tracer sample
    int steps;
    const float *velocity;   // a step: the velocity it leaves; an advance: the one it reads
    const sfl::BatchMember *records;
    float dt;
    float *trail;
    sfl::TracerGrid grid;
    int field;
};
static std::vector<Event> events;

static hipError_t note_step(char kind, const sfl::BatchStep &a, const sfl::BatchMember *records)
{
    events.push_back({kind, 1, a.step.v_out, records, a.step.dt, nullptr, {}, -1});
    return hipSuccess;
}

namespace sfl {
bool small_grid_fits(int dim_x, int dim_y)   // (the real rule of small_grid.hip; launch_stubs_ok.cpp's answer is "no")
{
    return dim_x >= 2 && dim_y >= 2 && (long long)dim_x * dim_y <= kSmallGridMaxCells &&
           (long long)dim_y * ((dim_x + 1) / 2) <= kSmallGridMaxCells / 2;
}
hipError_t launch_project_advect_vec3uq32(hipStream_t, uint32_t *, const uint32_t *, float *vel, const float *, Slab, int, int, int, int, float dt, bool, int *, float,
                                          int, bool *)
{
    events.push_back({'P', 1, vel, nullptr, dt, nullptr, {}, -1});
    return hipSuccess;
}
hipError_t launch_step_seam_tiled(hipStream_t, uint32_t *, const uint32_t *, float *next_v, float *, const float *, const float *, Slab, float dt, float)
{
    events.push_back({'M', 1, next_v, nullptr, dt, nullptr, {}, -1});
    return hipSuccess;
}
hipError_t launch_batch_step(hipStream_t, const BatchStep &a, int) { return note_step('s', a, nullptr); }
hipError_t launch_batch_step_each(hipStream_t, const BatchStep &a, int, const BatchMember *m, float *) { return note_step('e', a, m); }
hipError_t launch_batch_step_until(hipStream_t, const BatchStep &a, int, const BatchMember *m, const BatchStop *, float *, int *, bool) { return note_step('u', a, m); }
hipError_t launch_batch_large_step(hipStream_t, const BatchStep &a, int) { return note_step('s', a, nullptr); }
hipError_t launch_batch_large_step_each(hipStream_t, const BatchStep &a, int, const BatchMember *m, float *) { return note_step('e', a, m); }
hipError_t launch_batch_large_step_until(hipStream_t, const BatchStep &a, int, const BatchMember *m, const BatchStop *, float *, int *, bool) { return note_step('u', a, m); }
hipError_t launch_batch_play(hipStream_t, const BatchPlay &a, int, const BatchMember *m, float *)
{
    events.push_back({'p', a.steps, a.step.v_out, m, a.step.dt, nullptr, {}, -1});
    return hipSuccess;
}
hipError_t launch_batch_solve(hipStream_t, float *, const float *, int, int, int, int, SorParams) { return hipSuccess; }
hipError_t launch_batch_solve_each(hipStream_t, float *, const float *, int, int, int, const BatchMember *, float *) { return hipSuccess; }
hipError_t launch_batch_solve_until(hipStream_t, float *, const float *, int, int, int, const BatchMember *, const BatchStop *, float *, int *) { return hipSuccess; }
hipError_t launch_batch_large_solve(hipStream_t, float *, const float *, int, int, int, int, SorParams) { return hipSuccess; }
hipError_t launch_batch_large_solve_each(hipStream_t, float *, const float *, int, int, int, const BatchMember *, float *) { return hipSuccess; }
hipError_t launch_batch_large_solve_until(hipStream_t, float *, const float *, int, int, int, const BatchMember *, const BatchStop *, float *, int *) { return hipSuccess; }
hipError_t launch_batch_render(hipStream_t, uint16_t *, const uint32_t *, int, int, int, int, bool) { return hipSuccess; }
hipError_t launch_flow_stats(hipStream_t, FlowStatsRecord *, int, const float *, const uint32_t *, int, int, int, float, const float *) { return hipSuccess; }
// an advance adds 1 to every x (so a download shows how many ran) and copies the positions to the slot it is handed
hipError_t launch_tracer_advance(hipStream_t, const TracerGrid &g, const float *velocity, const BatchMember *records, float dt, float *trail)
{
    events.push_back({'A', 1, velocity, records, dt, trail, g, -1});
    const size_t all = (size_t)g.members * g.count;
    for (size_t k = 0; k < all; ++k) g.xy[2 * k] += 1.0f;
    if (trail) memcpy(trail, g.xy, all * 8);
    return hipSuccess;
}
// every byte of the samples gets 0x40 + field
hipError_t launch_tracer_sample(hipStream_t, const TracerGrid &g, int field, const void *of_first_member, bool, void *out)
{
    events.push_back({'Q', 0, static_cast<const float *>(of_first_member), nullptr, 0.0f, nullptr, g, field});
    const size_t elem = field == SFL_FIELD_VELOCITY ? 8 : field == SFL_FIELD_COLOR ? 12 : 4;
    memset(out, 0x40 + field, (size_t)g.members * g.count * elem);
    return hipSuccess;
}
}  // namespace sfl

static const float DT = 0.03f, DX = 1.0f, OMEGA = 1.9f;
static bool says(const char *word) { return strstr(sfl_last_error(), word) != nullptr; }

static std::string kinds()
{
    std::string s;
    for (const Event &e : events) s += e.kind;
    return s;
}

static void refusals_without_handles()
{
    float xy[4] = {0, 0, 1, 1};
    size_t n = 7;
    int w = 0;
    CHECK(sfl_tracers_set(nullptr, xy, 2, 1) == SFL_ERR_INVALID && says("sfl_tracers_set") && says("NULL"), "set: %s", sfl_last_error());
    CHECK(sfl_batch_tracers_set(nullptr, xy, 2, 1) == SFL_ERR_INVALID && says("sfl_batch_tracers_set"), "batch set: %s", sfl_last_error());
    CHECK(sfl_tracers_count(nullptr, &n) == SFL_ERR_INVALID && sfl_batch_tracers_count(nullptr, &n) == SFL_ERR_INVALID && n == 7, "count");
    CHECK(sfl_tracers_download(nullptr, xy, 4) == SFL_ERR_INVALID && sfl_batch_tracers_download(nullptr, xy, 4) == SFL_ERR_INVALID && says("NULL"), "download");
    CHECK(sfl_tracers_advance(nullptr, DT) == SFL_ERR_INVALID && sfl_batch_tracers_advance(nullptr, DT) == SFL_ERR_INVALID && says("NULL"), "advance");
    CHECK(sfl_tracers_sample(nullptr, 4, 0, xy, 16) == SFL_ERR_INVALID && says("unknown field id 4"), "field 4: %s", sfl_last_error());
    CHECK(sfl_batch_tracers_sample(nullptr, -1, 0, xy, 16) == SFL_ERR_INVALID && says("unknown field id -1"), "field -1: %s", sfl_last_error());
    CHECK(sfl_tracers_sample(nullptr, 0, 0, xy, 16) == SFL_ERR_INVALID && says("NULL"), "sample NULL: %s", sfl_last_error());
    CHECK(sfl_tracers_trail_start(nullptr, 0, 4) == SFL_ERR_INVALID && says("every must be >= 1"), "every 0: %s", sfl_last_error());
    CHECK(sfl_batch_tracers_trail_start(nullptr, -2, 4) == SFL_ERR_INVALID && says("got -2"), "every -2: %s", sfl_last_error());
    CHECK(sfl_tracers_trail_start(nullptr, 1, 0) == SFL_ERR_INVALID && says("capacity must be >= 1"), "capacity 0: %s", sfl_last_error());
    CHECK(sfl_tracers_trail_start(nullptr, 1, 1) == SFL_ERR_INVALID && says("NULL"), "trail_start NULL: %s", sfl_last_error());
    CHECK(sfl_tracers_trail_stop(nullptr) == SFL_ERR_INVALID && sfl_tracers_trail_info(nullptr, &w, &w, nullptr) == SFL_ERR_INVALID, "stop, info");
    CHECK(sfl_tracers_trail_read(nullptr, -1, 1, xy, 4) == SFL_ERR_INVALID && says("must be >= 0"), "first_slot -1: %s", sfl_last_error());
    CHECK(sfl_batch_tracers_trail_read(nullptr, 0, 1, xy, 4) == SFL_ERR_INVALID && says("NULL"), "read NULL: %s", sfl_last_error());
    CHECK(events.empty(), "a refused call launches nothing");
}

static bool trail_is(sfl_context *c, int written, int capacity, int64_t advances)
{
    int w = -1, cap = -1;
    int64_t a = -1;
    return sfl_tracers_trail_info(c, &w, &cap, &a) == SFL_OK && w == written && cap == capacity && a == advances;
}
static bool trail_is(sfl_batch *b, int written, int capacity, int64_t advances)
{
    int w = -1, cap = -1;
    int64_t a = -1;
    return sfl_batch_tracers_trail_info(b, &w, &cap, &a) == SFL_OK && w == written && cap == capacity && a == advances;
}

// every step event is followed by one advance on the velocity it left, with these records and this dt
static bool each_step_followed(const char *step_kinds, const sfl::BatchMember *records, bool dt_matters, float dt)
{
    if (events.empty() || events.size() % 2) return false;
    for (size_t k = 0; k < events.size(); k += 2) {
        const Event &s = events[k], &a = events[k + 1];
        if (!strchr(step_kinds, s.kind) || s.steps != 1 || a.kind != 'A') return false;
        if (a.velocity != s.velocity || a.records != records) return false;
        if (dt_matters && a.dt != dt) return false;
    }
    return true;
}

static void contexts()
{
    sfl_context *c = nullptr, *small = nullptr, *slab = nullptr;
    CHECK(sfl_create(&c, 0, 160, 128) == SFL_OK && sfl_create(&small, 0, 16, 12) == SFL_OK && sfl_create_slab(&slab, 0, 160, 128, 0, 2) == SFL_OK,
          "create: %s", sfl_last_error());
    if (!c || !small || !slab) return;
    const int N = 5;
    float xy[2 * N], back[2 * N];
    for (int k = 0; k < 2 * N; ++k) xy[k] = 10.0f * k;
    size_t n = 99;
    // ---- refusals
    CHECK(sfl_tracers_set(slab, xy, N, 1) == SFL_ERR_STATE && says("whole-domain"), "a slab: %s", sfl_last_error());
    CHECK(sfl_tracers_advance(slab, DT) == SFL_ERR_STATE && sfl_tracers_trail_start(slab, 1, 1) == SFL_ERR_STATE, "a slab");
    CHECK(sfl_tracers_set(c, nullptr, N, 1) == SFL_ERR_INVALID && says("xy is NULL"), "xy NULL: %s", sfl_last_error());
    CHECK(sfl_tracers_count(c, &n) == SFL_OK && n == 0 && c->tracers_follow == nullptr, "no set yet");
    CHECK(sfl_tracers_download(c, back, 2 * N) == SFL_ERR_STATE && says("no tracers attached"), "download without a set: %s", sfl_last_error());
    CHECK(sfl_tracers_advance(c, DT) == SFL_ERR_STATE && says("no tracers attached"), "advance without a set");
    CHECK(sfl_tracers_sample(c, SFL_FIELD_PRESSURE, 0, back, sizeof back) == SFL_ERR_STATE && says("no tracers attached"), "sample without a set");
    CHECK(sfl_tracers_trail_start(c, 1, 4) == SFL_ERR_STATE && says("a trail needs a set"), "trail without a set: %s", sfl_last_error());
    CHECK(sfl_tracers_trail_read(c, 0, 0, back, 0) == SFL_ERR_STATE && says("no trail"), "read without a trail: %s", sfl_last_error());
    CHECK(sfl_tracers_trail_stop(c) == SFL_OK && trail_is(c, 0, 0, 0), "stop without a trail is fine");
    CHECK(events.empty() && fake_hip_live_allocations() > 0, "nothing launched");

    // ---- without a set, and with a set that does not follow: the launches of before (three seams, then a stored projection)
    CHECK(sfl_step_n(c, 4, DT, DX, 3, OMEGA) == SFL_OK && kinds() == "MMMP", "step_n(4) without a set: %s (%s)", kinds().c_str(), sfl_last_error());
    events.clear();
    CHECK(sfl_tracers_set(c, xy, N, 0) == SFL_OK && sfl_tracers_count(c, &n) == SFL_OK && n == N && c->tracers_follow == nullptr, "a set that does not follow");
    CHECK(sfl_step_n(c, 4, DT, DX, 3, OMEGA) == SFL_OK && kinds() == "MMMP", "... is not advanced by steps: %s", kinds().c_str());
    CHECK(sfl_tracers_download(c, back, 2 * N) == SFL_OK && memcmp(back, xy, sizeof xy) == 0, "the positions as set");
    CHECK(sfl_tracers_download(c, back, 2 * N - 1) == SFL_ERR_INVALID && says("10 floats") && sfl_tracers_download(c, nullptr, 2 * N) == SFL_ERR_INVALID, "capacity: %s", sfl_last_error());
    events.clear();
    CHECK(sfl_tracers_advance(c, 0.5f) == SFL_OK && kinds() == "A" && events[0].velocity == c->vel && events[0].dt == 0.5f && events[0].records == nullptr &&
              events[0].trail == nullptr, "a manual advance on the context's velocity");
    CHECK(events[0].grid.count == (unsigned)N && events[0].grid.members == 1 && events[0].grid.dim_x == 160 && events[0].grid.dim_y == 128 &&
              events[0].grid.member_cells == 160u * 128u && events[0].grid.xy == c->tracers.d_xy, "the grid of a context");
    // ---- samples
    uint8_t out[12 * N + 1];
    for (int field = 0; field < 4; ++field) {
        const size_t bytes = (size_t)N * (field == 0 ? 8 : field == 1 ? 12 : 4);
        memset(out, 0, sizeof out);
        events.clear();
        CHECK(sfl_tracers_sample(c, field, 1, out, bytes) == SFL_OK && kinds() == "Q" && events[0].field == field, "sample of field %d: %s", field, sfl_last_error());
        CHECK(out[0] == 0x40 + field && out[bytes - 1] == 0x40 + field && out[bytes] == 0, "field %d: exactly its bytes copied out", field);
        CHECK(sfl_tracers_sample(c, field, 1, out, bytes - 1) == SFL_ERR_INVALID && says("capacity"), "field %d: capacity too small: %s", field, sfl_last_error());
    }
    CHECK(events[0].velocity == c->p, "the pressure sampled is the context's current pressure");
    CHECK(sfl_tracers_sample(c, 7, 1, out, sizeof out) == SFL_ERR_INVALID && says("unknown field") && sfl_tracers_sample(c, 0, 1, nullptr, 99) == SFL_ERR_INVALID, "field 7, NULL");

    // ---- a following set: no seams, one advance behind every step, on the velocity the step left
    events.clear();
    CHECK(sfl_tracers_set(c, xy, N, 1) == SFL_OK && c->tracers_follow != nullptr, "a following set replaces the other");
    CHECK(sfl_step_n(c, 4, DT, DX, 3, OMEGA) == SFL_OK && kinds() == "PAPAPAPA" && each_step_followed("P", nullptr, true, DT), "step_n(4): %s", kinds().c_str());
    CHECK(events.back().velocity == c->vel && events.back().trail == nullptr, "the last advance read the velocity the context holds");
    CHECK(sfl_tracers_download(c, back, 2 * N) == SFL_OK && back[0] == xy[0] + 4 && back[1] == xy[1], "four advances ran");
    events.clear();
    CHECK(sfl_step(c, DT, DX, 3, OMEGA) == SFL_OK && kinds() == "PA", "sfl_step: %s", kinds().c_str());
    // ---- trails: every = 2, three slots
    CHECK(sfl_tracers_trail_start(c, 2, 3) == SFL_OK && trail_is(c, 0, 3, 0), "trail_start: %s", sfl_last_error());
    events.clear();
    CHECK(sfl_step_n(c, 3, DT, DX, 3, OMEGA) == SFL_OK && kinds() == "PAPAPA" && trail_is(c, 1, 3, 3), "three steps: one slot");
    CHECK(events[1].trail == nullptr && events[3].trail == c->tracers.d_trail && events[5].trail == nullptr, "the second advance writes slot 0");
    CHECK(sfl_tracers_advance(c, DT) == SFL_OK && trail_is(c, 2, 3, 4) && events.back().trail == c->tracers.d_trail + 2 * N, "a manual advance counts: slot 1");
    events.clear();
    CHECK(sfl_step_n(c, 4, DT, DX, 3, OMEGA) == SFL_ERR_STATE && says("room for 1 more") && events.empty() && trail_is(c, 2, 3, 4), "overflow is refused whole: %s", sfl_last_error());
    CHECK(sfl_step_n(c, 3, DT, DX, 3, OMEGA) == SFL_OK && trail_is(c, 3, 3, 7), "three more steps fit");
    CHECK(sfl_step(c, DT, DX, 3, OMEGA) == SFL_ERR_STATE && sfl_tracers_advance(c, DT) == SFL_ERR_STATE && trail_is(c, 3, 3, 7), "a full trail refuses step and advance");
    float slots[3 * 2 * N];
    CHECK(sfl_tracers_trail_read(c, 0, 3, slots, 3 * 2 * N) == SFL_OK && slots[0] == xy[0] + 7 && slots[2 * N] == xy[0] + 9 && slots[4 * N] == xy[0] + 11 &&
              slots[1] == xy[1], "the slots hold the positions after advances 2, 4 and 6 of the trail");
    CHECK(sfl_tracers_trail_read(c, 1, 3, slots, 3 * 2 * N) == SFL_ERR_INVALID && says("not inside the 3 slots written"), "a range outside: %s", sfl_last_error());
    CHECK(sfl_tracers_trail_read(c, 0, 2, slots, 4 * N - 1) == SFL_ERR_INVALID && says("20 floats") && sfl_tracers_trail_read(c, 0, 1, nullptr, 99) == SFL_ERR_INVALID, "capacity, NULL");
    CHECK(sfl_tracers_trail_start(c, 1, 2) == SFL_OK && trail_is(c, 0, 2, 0), "started afresh");
    CHECK(sfl_tracers_trail_stop(c) == SFL_OK && trail_is(c, 0, 0, 0) && c->tracers.d_trail == nullptr && sfl_step(c, DT, DX, 3, OMEGA) == SFL_OK, "stop frees the slots");
    // ---- remove: the launches of before again
    CHECK(sfl_tracers_trail_start(c, 1, 2) == SFL_OK && sfl_tracers_set(c, nullptr, 0, 1) == SFL_OK && c->tracers_follow == nullptr && c->tracers.d_xy == nullptr &&
              c->tracers.d_trail == nullptr && trail_is(c, 0, 0, 0), "n == 0 removes the set and its trail");
    events.clear();
    CHECK(sfl_step_n(c, 3, DT, DX, 3, OMEGA) == SFL_OK && kinds() == "MMP", "the seams are back: %s", kinds().c_str());
    // ---- the one-workgroup path of a context: the hook is the same
    events.clear();
    CHECK(sfl_tracers_set(small, xy, N, 1) == SFL_OK && sfl_step_n(small, 3, DT, DX, 3, OMEGA) == SFL_OK && kinds() == "AAA" && events[2].velocity == small->vel,
          "a small context: %s (%s)", kinds().c_str(), sfl_last_error());
    // ---- destroy with a live set and a live trail
    CHECK(sfl_tracers_set(c, xy, N, 1) == SFL_OK && sfl_tracers_trail_start(c, 1, 8) == SFL_OK && sfl_step(c, DT, DX, 3, OMEGA) == SFL_OK, "a live trail");
    for (sfl_context *x : {c, small, slab}) CHECK(sfl_destroy(x) == SFL_OK, "destroy");
    events.clear();
}

static void batches(bool large)
{
    const int B = 4, K = 3, X = 8, Y = 6;
    sfl_batch *b = nullptr;
    CHECK((large ? sfl_batch_create_large : sfl_batch_create)(&b, 0, X, Y, B) == SFL_OK && b, "create: %s", sfl_last_error());
    if (!b) return;
    float xy[B * K * 2], back[B * K * 2];
    for (int k = 0; k < B * K * 2; ++k) xy[k] = 0.25f * k;
    sfl_member_params prm[B];
    sfl_member_stop stop[B];
    for (int m = 0; m < B; ++m) {
        prm[m] = {DT * (m + 1), DX, OMEGA, 3 + m};
        stop[m] = {-1.0f, 2};
    }
    const int m1[1] = {1}, cell[2] = {1, 1};
    const float vel[2] = {1.f, 0.f};
    // ---- without a set: one launch per step, the replay of a timeline in one launch (small members), no tracer launch
    events.clear();
    CHECK(sfl_batch_step_n(b, 2, DT, DX, 3, OMEGA) == SFL_OK && sfl_batch_step_n_each(b, 2, prm) == SFL_OK && sfl_batch_step_n_until(b, 2, prm, stop) == SFL_OK &&
              kinds() == "sseeuu", "without a set: %s", kinds().c_str());
    events.clear();
    CHECK(sfl_batch_queue_forces_at(b, 2, m1, cell, vel, 1) == SFL_OK && sfl_batch_step_n(b, 4, DT, DX, 3, OMEGA) == SFL_OK && kinds() == (large ? "ssss" : "p"),
          "the replay without a set: %s", kinds().c_str());
    // ---- a set that does not follow changes nothing
    size_t k = 0;
    CHECK(sfl_batch_tracers_set(b, xy, K, 0) == SFL_OK && sfl_batch_tracers_count(b, &k) == SFL_OK && k == K && b->tracers_follow == nullptr, "a set that does not follow");
    events.clear();
    CHECK(sfl_batch_queue_forces_at(b, 2, m1, cell, vel, 1) == SFL_OK && sfl_batch_step_n_each(b, 3, prm) == SFL_OK && kinds() == (large ? "eee" : "p"),
          "... is not advanced: %s", kinds().c_str());
    CHECK(sfl_batch_tracers_download(b, back, B * K * 2) == SFL_OK && memcmp(back, xy, sizeof xy) == 0, "the positions as set");
    CHECK(sfl_batch_tracers_download(b, back, B * K * 2 - 1) == SFL_ERR_INVALID && says("24 floats"), "capacity counts every member: %s", sfl_last_error());
    events.clear();
    CHECK(sfl_batch_tracers_advance(b, 0.5f) == SFL_OK && kinds() == "A" && events[0].velocity == b->vel && events[0].records == nullptr && events[0].dt == 0.5f, "a manual advance");
    CHECK(events[0].grid.count == (unsigned)K && events[0].grid.members == B && events[0].grid.dim_x == X && events[0].grid.dim_y == Y && events[0].grid.member_cells == (size_t)X * Y,
          "the grid of a batch");
    uint32_t dye[B * K * 3];
    events.clear();
    CHECK(sfl_batch_tracers_sample(b, SFL_FIELD_COLOR, 0, dye, sizeof dye) == SFL_OK && kinds() == "Q" && (const void *)events[0].velocity == (const void *)b->col &&
              dye[B * K * 3 - 1] == 0x41414141u, "a sample of the dye: %s", sfl_last_error());
    CHECK(sfl_batch_tracers_sample(b, SFL_FIELD_COLOR, 0, dye, sizeof dye - 4) == SFL_ERR_INVALID && says("144 bytes"), "capacity: %s", sfl_last_error());
    // ---- a following set: one advance behind every step, with the call's records (each, until) or its dt (uniform)
    CHECK(sfl_batch_tracers_set(b, xy, K, 1) == SFL_OK && b->tracers_follow != nullptr, "a following set");
    events.clear();
    CHECK(sfl_batch_step_n(b, 3, DT, DX, 3, OMEGA) == SFL_OK && kinds() == "sAsAsA" && each_step_followed("s", nullptr, true, DT), "step_n: %s", kinds().c_str());
    CHECK(events.back().velocity == b->vel, "the last advance read the velocity the batch holds");
    events.clear();
    CHECK(sfl_batch_step_n_each(b, 2, prm) == SFL_OK && kinds() == "eAeA" && each_step_followed("e", b->d_members, false, 0) && b->d_members, "step_n_each: %s", kinds().c_str());
    events.clear();
    CHECK(sfl_batch_step_n_until(b, 2, prm, stop) == SFL_OK && kinds() == "uAuA" && each_step_followed("u", b->d_members, false, 0), "step_n_until: %s", kinds().c_str());
    {   // the records hold every member once, most iterations first, each with its own dt
        bool seen[B] = {false, false, false, false}, ok = true;
        for (int r = 0; r < B; ++r) {
            const sfl::BatchMember &rec = b->d_members[r];
            ok = ok && rec.member >= 0 && rec.member < B && !seen[rec.member] && rec.dt == prm[rec.member].dt;
            if (rec.member >= 0 && rec.member < B) seen[rec.member] = true;
        }
        CHECK(ok && b->d_members[0].member == B - 1, "the member table the advance reads");
    }
    // ---- the replay runs no step unseen: a record at step 2 of 4, per-step launches with the advance behind each
    events.clear();
    CHECK(sfl_batch_queue_forces_at(b, 2, m1, cell, vel, 1) == SFL_OK && sfl_batch_step_n(b, 4, DT, DX, 3, OMEGA) == SFL_OK && kinds() == "sAsAsAsA" &&
              each_step_followed("s", nullptr, true, DT), "a timeline with a following set: %s", kinds().c_str());
    events.clear();
    CHECK(sfl_batch_queue_forces_at(b, 1, m1, cell, vel, 1) == SFL_OK && sfl_batch_step_n_each(b, 3, prm) == SFL_OK && kinds() == "eAeAeA" &&
              each_step_followed("e", b->d_members, false, 0), "... by step_n_each: %s", kinds().c_str());
    CHECK(sfl_batch_tracers_download(b, back, B * K * 2) == SFL_OK && back[0] == xy[0] + 14 && back[1] == xy[1], "14 advances ran since the set");
    // ---- trails, with the recorder alongside
    CHECK(sfl_batch_record_start(b, 2, 0, B, 1, 1, 8) == SFL_OK && sfl_batch_tracers_trail_start(b, 1, 3) == SFL_OK && trail_is(b, 0, 3, 0), "trail: %s", sfl_last_error());
    events.clear();
    CHECK(sfl_batch_step_n(b, 2, DT, DX, 3, OMEGA) == SFL_OK && kinds() == "sAsA" && trail_is(b, 2, 3, 2) && events[1].trail == b->tracers.d_trail &&
              events[3].trail == b->tracers.d_trail + B * K * 2, "every = 1: a slot per step, a slot the positions of every member");
    events.clear();
    int frames = -1;
    CHECK(sfl_batch_step_n_each(b, 2, prm) == SFL_ERR_STATE && says("room for 1 more") && events.empty() && trail_is(b, 2, 3, 2) &&
              sfl_batch_record_info(b, &frames, nullptr, nullptr) == SFL_OK && frames == 1, "overflow is refused whole: %s", sfl_last_error());
    CHECK(sfl_batch_step_n_until(b, 2, prm, stop) == SFL_ERR_STATE && sfl_batch_step_n(b, 2, DT, DX, 3, OMEGA) == SFL_ERR_STATE && events.empty(), "... by every step call");
    CHECK(sfl_batch_tracers_advance(b, DT) == SFL_OK && trail_is(b, 3, 3, 3) && sfl_batch_tracers_advance(b, DT) == SFL_ERR_STATE, "a manual advance fills the trail");
    float slots[3 * B * K * 2];
    CHECK(sfl_batch_tracers_trail_read(b, 1, 2, slots, 2 * B * K * 2) == SFL_OK && slots[0] == xy[0] + 16 && slots[B * K * 2] == xy[0] + 17, "slots 1 and 2");
    CHECK(sfl_batch_tracers_trail_read(b, 2, 2, slots, sizeof slots / 4) == SFL_ERR_INVALID && says("not inside"), "a range outside: %s", sfl_last_error());
    // ---- replace with a live trail, then destroy with a live trail
    CHECK(sfl_batch_tracers_set(b, xy, 2, 1) == SFL_OK && trail_is(b, 0, 0, 0) && b->tracers.d_trail == nullptr, "a new set ends the trail");
    CHECK(sfl_batch_tracers_trail_start(b, 3, 2) == SFL_OK && sfl_batch_step_n(b, 3, DT, DX, 3, OMEGA) == SFL_OK && trail_is(b, 1, 2, 3), "a live trail: %s", sfl_last_error());
    CHECK(sfl_batch_destroy(b) == SFL_OK, "destroy");
    events.clear();
}

int main()
{
    refusals_without_handles();
    contexts();
    batches(false);
    batches(true);
    const long left = fake_hip_live_allocations();
    printf("tracers driver: %d failed checks, %ld allocations left\n", failures, left);
    return failures || left ? 1 : 0;
}
