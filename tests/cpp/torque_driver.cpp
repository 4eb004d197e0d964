// torque_driver.cpp -- TEST HARNESS (tests/cpp, `make -f torque.mk`; tests/test_torque.py).  Two programs in one:
//   torque_driver                  the HOST side of the torque (csrc/torque.cpp, csrc/body_recorder.h) and of its hooks in the step
//                                  calls (csrc/batch.cpp, csrc/slab_step.cpp), run on a box without a GPU: the host units over the
//                                  runtime that lives on the host (fake_hip.cpp) and kernels that do nothing (launch_stubs_ok.cpp).
//                                  The launchers of the batches, of the solids, of the histories, of the loads, of the friction and
//                                  of the torque are stubs of THIS file that keep ONE log in the order of the calls, which is the
//                                  order of the stream.  What is checked: the argument refusals in the loads' order, each with the
//                                  call's own name; the pivots' calls; torque_admit refusing a call whole at all five admission
//                                  points; samples without solids (zeros and the pivots) inside a one-launch replay and across the
//                                  seams of sfl_step_n, neither of which is cut; the order history, loads, friction, torque behind
//                                  a step; what the samplers are handed; sfl_[batch_]set_bodies refused while the torque recorder
//                                  is on, with its own message; with no torque recorder the launch log of every step call identical
//                                  to the one made while the unit's pointer was still null; destroy leaves no allocation.
//   torque_driver <in> <out>       csrc/torque_face.h face by face: <in> holds records of nine int64 (i, j, dir, px2, py2, tp, tf,
//                                  faces, max_arm2), <out> gets eight int64 per record (rx2, ry2, the longest arm, the pressure
//                                  product, the friction product, L(faces), L(max_arm2), s), which the test compares with
//                                  tests/torque_rule.py.
// Exit status 0 and "0 failed checks".
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../esp32-fluid-simulation_amd/csrc/batch_state.h"
#include "../../esp32-fluid-simulation_amd/csrc/friction_kernels.h"
#include "../../esp32-fluid-simulation_amd/csrc/history_kernels.h"
#include "../../esp32-fluid-simulation_amd/csrc/load_kernels.h"
#include "../../esp32-fluid-simulation_amd/csrc/solid_kernels.h"
#include "../../esp32-fluid-simulation_amd/csrc/torque_face.h"
#include "../../esp32-fluid-simulation_amd/csrc/torque_kernels.h"
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
// 'C' a context's; 'F' a batch's friction sample, 'X' a context's; 'T' a batch's torque sample, 'Y' a context's, 'Z' the
// torque's sample without solids (n: the records)
struct Event {
    char kind;
    int n;
    sfl::BatchTorqueSample batch;
    sfl::ContextTorqueSample context;
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
    memset(a.out, 0x3c, sizeof(struct sfl_body_load) * (size_t)a.count * a.bodies);
    return note('L', a.count);
}
hipError_t launch_context_loads(hipStream_t, const ContextLoadSample &a)
{
    memset(a.out, 0x3c, sizeof(struct sfl_body_load) * (size_t)a.bodies);
    return note('C', a.bodies);
}
hipError_t launch_batch_friction(hipStream_t, const BatchFrictionSample &a)
{
    memset(a.out, 0x5a, sizeof(struct sfl_body_friction) * (size_t)a.count * a.bodies);
    return note('F', a.count);
}
hipError_t launch_context_friction(hipStream_t, const ContextFrictionSample &a)
{
    memset(a.out, 0x5a, sizeof(struct sfl_body_friction) * (size_t)a.bodies);
    return note('X', a.bodies);
}
hipError_t launch_batch_torque(hipStream_t, const BatchTorqueSample &a)
{
    memset(a.out, 0x6b, sizeof(struct sfl_body_torque) * (size_t)a.count * a.bodies);
    events.push_back({'T', a.count, a, {}});
    return hipSuccess;
}
hipError_t launch_context_torque(hipStream_t, const ContextTorqueSample &a)
{
    memset(a.out, 0x6b, sizeof(struct sfl_body_torque) * (size_t)a.bodies);
    events.push_back({'Y', a.bodies, {}, a});
    return hipSuccess;
}
// (what torque.hip's kernel does: zeros and the pivots)
hipError_t launch_torque_empty(hipStream_t, struct sfl_body_torque *out, const int32_t *pivot2, size_t pivot_stride, int first, int count, int bodies)
{
    memset(out, 0, sizeof(struct sfl_body_torque) * (size_t)count * bodies);
    for (int m = 0; m < count && pivot2; ++m)
        for (int k = 0; k < bodies; ++k) memcpy(out[(size_t)m * bodies + k].pivot2, pivot2 + (size_t)(first + m) * pivot_stride + 2 * k, 8);
    return note('Z', count * bodies);
}
}  // namespace sfl

static const float DT = 0.03f, DX = 0.7f, OMEGA = 1.9f;
static bool says(const char *word) { return strstr(sfl_last_error(), word) != nullptr; }
static std::string kinds(bool with_empty = true)
{
    std::string s;
    for (const Event &e : events)
        if (with_empty || e.kind != 'Z') s += e.kind;
    return s;
}
static bool all_bytes(const void *p, size_t n, int v)
{
    for (size_t k = 0; k < n; ++k)
        if (static_cast<const uint8_t *>(p)[k] != (uint8_t)v) return false;
    return true;
}
// zero records with these pivots (null: zeros), member-major from member `first` (stride 0: shared)
static bool zeros_and_pivots(const struct sfl_body_torque *rec, int count, int bodies, const int32_t *pivot2, int stride, int first)
{
    for (int m = 0; m < count; ++m)
        for (int k = 0; k < bodies; ++k) {
            struct sfl_body_torque want;
            memset(&want, 0, sizeof want);
            if (pivot2) memcpy(want.pivot2, pivot2 + (size_t)(first + m) * stride + 2 * k, 8);
            if (memcmp(&want, &rec[m * bodies + k], sizeof want)) return false;
        }
    return true;
}

static const int B = 3, X = 4, Y = 3, CELLS = X * Y;
static const uint8_t MASK[CELLS] = {0, 1, 0, 0, 0, 0, 7, 0, 0, 0, 0, 1};
static const size_t REC = sizeof(struct sfl_body_torque);

template <class H>
static bool info_is(H *x, int (*info)(H *, int *, int *, int64_t *, int *), int samples, int capacity, int64_t steps, int bodies)
{
    int s = -1, c = -1, n = -1;
    int64_t t = -1;
    const bool ok = info(x, &s, &c, &t, &n) == SFL_OK && s == samples && c == capacity && t == steps && n == bodies;
    if (!ok) fprintf(stderr, "  info: %d samples, capacity %d, %lld steps, %d bodies\n", s, c, (long long)t, n);
    return ok;
}

// the loads' refusals, in the loads' order, with each call's own name
static void refusals_without_handles()
{
    struct sfl_body_torque rec[4];
    int32_t piv[2] = {0, 0};
    int w = 5;
    CHECK(sfl_batch_torque(nullptr, 0, 1, rec, REC) == SFL_ERR_INVALID && says("sfl_batch_torque: batch is NULL"), "%s", sfl_last_error());
    CHECK(sfl_batch_torque_start(nullptr, 0, 0, 1, 1) == SFL_ERR_INVALID && says("sfl_batch_torque_start: every must be >= 1 (got 0)"), "%s", sfl_last_error());
    CHECK(sfl_batch_torque_start(nullptr, 1, 0, 1, 0) == SFL_ERR_INVALID && says("sfl_batch_torque_start: capacity must be >= 1 (got 0)"), "%s", sfl_last_error());
    CHECK(sfl_batch_torque_start(nullptr, 1, 0, 0, 1) == SFL_ERR_INVALID && says("sfl_batch_torque_start: count must be >= 1 (got 0)"), "%s", sfl_last_error());
    CHECK(sfl_batch_torque_start(nullptr, 1, 0, 1, 1) == SFL_ERR_INVALID && says("sfl_batch_torque_start: batch is NULL"), "%s", sfl_last_error());
    CHECK(sfl_batch_torque_stop(nullptr) == SFL_ERR_INVALID && says("sfl_batch_torque_stop: batch is NULL"), "%s", sfl_last_error());
    CHECK(sfl_batch_torque_info(nullptr, &w, &w, nullptr, &w) == SFL_ERR_INVALID && says("sfl_batch_torque_info: batch is NULL") && w == 5, "%s", sfl_last_error());
    CHECK(sfl_batch_torque_read(nullptr, -1, 0, rec, 0) == SFL_ERR_INVALID && says("sfl_batch_torque_read: samples [-1, -1 + 0): first_sample and samples must be >= 0"), "%s", sfl_last_error());
    CHECK(sfl_batch_torque_read(nullptr, 0, 0, rec, 0) == SFL_ERR_INVALID && says("sfl_batch_torque_read: batch is NULL"), "%s", sfl_last_error());
    CHECK(sfl_torque(nullptr, rec, REC) == SFL_ERR_INVALID && says("sfl_torque: ctx is NULL"), "%s", sfl_last_error());
    CHECK(sfl_torque_start(nullptr, 0, 1) == SFL_ERR_INVALID && says("sfl_torque_start: every must be >= 1"), "%s", sfl_last_error());
    CHECK(sfl_torque_start(nullptr, 1, 0) == SFL_ERR_INVALID && says("sfl_torque_start: capacity must be >= 1"), "%s", sfl_last_error());
    CHECK(sfl_torque_start(nullptr, 1, 1) == SFL_ERR_INVALID && says("sfl_torque_start: ctx is NULL"), "%s", sfl_last_error());
    CHECK(sfl_torque_stop(nullptr) == SFL_ERR_INVALID && says("sfl_torque_stop: ctx is NULL"), "%s", sfl_last_error());
    CHECK(sfl_torque_info(nullptr, &w, &w, nullptr, &w) == SFL_ERR_INVALID && says("sfl_torque_info: ctx is NULL") && w == 5, "%s", sfl_last_error());
    CHECK(sfl_torque_read(nullptr, 0, -1, rec, 0) == SFL_ERR_INVALID && says("sfl_torque_read: samples [0, 0 + -1)"), "%s", sfl_last_error());
    CHECK(sfl_torque_read(nullptr, 0, 0, rec, 0) == SFL_ERR_INVALID && says("sfl_torque_read: ctx is NULL"), "%s", sfl_last_error());
    CHECK(sfl_batch_set_body_pivots(nullptr, piv, 2, 1) == SFL_ERR_INVALID && says("sfl_batch_set_body_pivots: per_member must be 0 or 1 (got 2)"), "%s", sfl_last_error());
    CHECK(sfl_batch_set_body_pivots(nullptr, piv, 0, 1) == SFL_ERR_INVALID && says("sfl_batch_set_body_pivots: batch is NULL"), "%s", sfl_last_error());
    CHECK(sfl_batch_body_pivots_download(nullptr, 0, 1, piv, 8) == SFL_ERR_INVALID && says("sfl_batch_body_pivots_download: batch is NULL"), "%s", sfl_last_error());
    CHECK(sfl_set_body_pivots(nullptr, piv, 1) == SFL_ERR_INVALID && says("sfl_set_body_pivots: ctx is NULL"), "%s", sfl_last_error());
    CHECK(sfl_body_pivots_download(nullptr, piv, 8) == SFL_ERR_INVALID && says("sfl_body_pivots_download: ctx is NULL"), "%s", sfl_last_error());
    CHECK(events.empty(), "a refused call launches nothing");
}

static void batches()
{
    sfl_batch *b = nullptr, *large = nullptr;
    CHECK(sfl_batch_create(&b, 0, X, Y, B) == SFL_OK && sfl_batch_create_large(&large, 0, X, Y, B) == SFL_OK && b && large, "create: %s", sfl_last_error());
    if (!b || !large) return;
    sfl_member_params prm[B];
    for (int m = 0; m < B; ++m) prm[m] = {DT * (m + 1), DX, OMEGA, 3 + m};
    struct sfl_body_torque rec[B * 3 * 4];
    struct sfl_body_load lrec[B * 3 * 4];
    struct sfl_body_friction frec[B * 3 * 4];
    const auto baseline = [&] { return sfl_batch_step_n(b, 2, DT, DX, 4, OMEGA) == SFL_OK && sfl_batch_step_n_each(b, 1, prm) == SFL_OK; };
    // ---- the unit's pointer is null: the log to compare with; no solids: zero records without a launch
    events.clear();
    CHECK(b->torque_step == nullptr && baseline() && kinds() == "sse" && b->torque_step == nullptr, "baseline: %s", kinds().c_str());
    const std::string log0 = kinds();
    events.clear();
    memset(rec, 0xff, sizeof rec);
    CHECK(sfl_batch_torque(b, 0, B, rec, B * REC) == SFL_OK && all_bytes(rec, B * REC, 0) && events.empty() && b->torque.d_records == nullptr,
          "no solids, no pivots: zeros, no launch, no allocation: %s", sfl_last_error());
    CHECK(sfl_batch_torque(b, 1, 3, rec, 3 * REC) == SFL_ERR_INVALID && says("sfl_batch_torque: members [1, 1 + 3) are not inside the batch's [0, 3)"), "range: %s", sfl_last_error());
    CHECK(sfl_batch_torque(b, 0, 2, rec, REC) == SFL_ERR_INVALID && says("sfl_batch_torque: 2 members of 1 records of 64 bytes are 128 bytes, got 64"), "bytes: %s", sfl_last_error());
    CHECK(sfl_batch_torque(b, 0, 2, nullptr, 2 * REC) == SFL_ERR_INVALID && says("sfl_batch_torque: host is NULL"), "host: %s", sfl_last_error());
    CHECK(sfl_batch_torque_read(b, 0, 0, rec, 0) == SFL_ERR_STATE && says("sfl_batch_torque_read: no torque recorder to read: call sfl_torque_start (sfl_batch_torque_start) first"),
          "read without: %s", sfl_last_error());
    // ---- the pivots: shared and per member, the bound, the number of bodies, NULL
    const int32_t shared[2] = {7, -3}, each[B * 2] = {1, 2, -3, -4, SFL_TORQUE_MAX_PIVOT2, -SFL_TORQUE_MAX_PIVOT2};
    int32_t got[B * 2], beyond[B * 2] = {0, 0, 0, -SFL_TORQUE_MAX_PIVOT2 - 1, 0, 0};
    CHECK(sfl_batch_body_pivots_download(b, 0, B, got, sizeof got) == SFL_OK && all_bytes(got, sizeof got, 0), "no pivots: zeros");
    CHECK(sfl_batch_set_body_pivots(b, shared, 0, 2) == SFL_ERR_INVALID && says("sfl_batch_set_body_pivots: bodies must be the 1 that sfl_batch_bodies_info reports (got 2)"), "bodies: %s", sfl_last_error());
    CHECK(sfl_batch_set_body_pivots(b, beyond, 1, 1) == SFL_ERR_INVALID && says("sfl_batch_set_body_pivots: pivot2[1] = -16777217 of body 1 of member 1 is beyond +-16777216 half cells") &&
              b->torque.d_pivot2 == nullptr, "the bound, per member: %s", sfl_last_error());
    beyond[0] = SFL_TORQUE_MAX_PIVOT2 + 1;
    CHECK(sfl_batch_set_body_pivots(b, beyond, 0, 1) == SFL_ERR_INVALID && says("pivot2[0] = 16777217 of body 1 is beyond") && !says("member"), "the bound, shared: %s", sfl_last_error());
    CHECK(sfl_batch_set_body_pivots(b, shared, 0, 1) == SFL_OK && b->torque.d_pivot2 && b->torque.d_pivot_bytes == 8 && !b->torque.pivots_per_member &&
              memcmp(b->torque.d_pivot2, shared, 8) == 0, "shared pivots: %s", sfl_last_error());
    CHECK(sfl_batch_body_pivots_download(b, 1, 2, got, 16) == SFL_OK && memcmp(got, shared, 8) == 0 && memcmp(got + 2, shared, 8) == 0, "shared pivots: repeated");
    CHECK(sfl_batch_body_pivots_download(b, 1, 2, got, 8) == SFL_ERR_INVALID && says("sfl_batch_body_pivots_download: the pivots of 1 bodies of 2 members are 16 bytes, got 8"), "%s", sfl_last_error());
    events.clear();
    CHECK(sfl_batch_torque(b, 1, 2, rec, 2 * REC) == SFL_OK && zeros_and_pivots(rec, 2, 1, shared, 0, 1) && events.empty(), "no solids: zeros and the pivots, no launch");
    CHECK(sfl_batch_set_body_pivots(b, each, 1, 1) == SFL_OK && b->torque.pivots_per_member && b->torque.d_pivot_bytes == sizeof each && memcmp(b->torque.d_pivot2, each, sizeof each) == 0,
          "pivots per member, at the bound: %s", sfl_last_error());
    CHECK(sfl_batch_torque(b, 1, 2, rec, 2 * REC) == SFL_OK && zeros_and_pivots(rec, 2, 1, each, 2, 1), "... of members 1 and 2");
    // ---- the recorder without solids: steps counted across calls, the samples zeros and the pivots
    CHECK(sfl_batch_torque_start(b, 2, 2, 2, 2) == SFL_ERR_INVALID && says("members [2, 2 + 2) are not inside the batch's [0, 3)") && !b->torque.on, "start: range: %s", sfl_last_error());
    CHECK(sfl_batch_torque_start(b, 2, 1, 2, 2) == SFL_OK && b->torque.on && b->torque_step && !b->loads.on && b->loads_step == nullptr && b->friction_step == nullptr &&
              info_is(b, sfl_batch_torque_info, 0, 2, 0, 1), "start: %s", sfl_last_error());
    CHECK(b->torque.d_bytes == (B + 2 * 2) * REC && b->loads.d_records == nullptr && b->friction.d_records == nullptr,
          "the records: one sample of every member in front, then capacity x count: %zu", b->torque.d_bytes);
    void *buffer = b->torque.d_records;
    memset(buffer, 0xff, b->torque.d_bytes);
    events.clear();
    CHECK(sfl_batch_step_n(b, 3, DT, DX, 4, OMEGA) == SFL_OK && kinds() == "ssZs" && info_is(b, sfl_batch_torque_info, 1, 2, 3, 1), "3 steps: %s", kinds().c_str());
    // the pivots change while the recorder is on: they hold from the next sample
    CHECK(sfl_batch_set_body_pivots(b, shared, 0, 1) == SFL_OK && b->torque.on && info_is(b, sfl_batch_torque_info, 1, 2, 3, 1), "pivots while recording: %s", sfl_last_error());
    CHECK(sfl_batch_step_n_each(b, 1, prm) == SFL_OK && kinds() == "ssZseZ" && info_is(b, sfl_batch_torque_info, 2, 2, 4, 1), "... and one more, by the _each call: %s", kinds().c_str());
    CHECK(sfl_batch_torque_read(b, 0, 2, rec, 2 * 2 * REC) == SFL_OK && zeros_and_pivots(rec, 2, 1, each, 2, 1) && zeros_and_pivots(rec + 2, 2, 1, shared, 0, 1),
          "sample 0 with the old pivots, sample 1 with the new ones");
    CHECK(all_bytes(buffer, B * REC, 0xff), "... and the room of the synchronous call is not a sample's");
    CHECK(sfl_batch_torque_read(b, 1, 2, rec, 4 * REC) == SFL_ERR_INVALID && says("not inside the 2 samples written so far"), "read: range: %s", sfl_last_error());
    CHECK(sfl_batch_torque_read(b, 0, 2, rec, 3 * REC) == SFL_ERR_INVALID && says("2 samples of 2 records of 64 bytes (2 members of 1 bodies) are 256 bytes, got 192"), "read: bytes: %s", sfl_last_error());
    // ---- full: the three step calls of a batch are refused whole, their own argument checks first (admission points 1 to 3)
    const int ms[2] = {0, 2}, cells[4] = {0, 0, 1, 0};
    const float vels[4] = {1, 0, 0, 1};
    CHECK(sfl_batch_queue_forces_at(b, 0, ms, cells, vels, 1) == SFL_OK, "a record to keep");
    events.clear();
    sfl::BatchMember *members_before = b->d_members;
    const int slot_before = b->member_slot;
    int pending = -1;
    CHECK(sfl_batch_step_n(b, 2, DT, DX, -1, OMEGA) == SFL_ERR_INVALID && says("iters must be >= 0"), "iters first: %s", sfl_last_error());
    CHECK(sfl_batch_step_n(b, 2, DT, DX, 4, OMEGA) == SFL_ERR_STATE && says("the torque recorder has room for 0 more samples (2 of 2 written) and 2 steps would complete 1") &&
              says("sfl_batch_torque_read"), "step_n while full: %s", sfl_last_error());
    CHECK(sfl_batch_step_n_each(b, 2, prm) == SFL_ERR_STATE && says("the torque recorder") && sfl_batch_step_n_each(b, 2, nullptr) == SFL_ERR_INVALID, "step_n_each while full");
    sfl_member_stop stop[B] = {{-1.0f, 2}, {-1.0f, 2}, {-1.0f, 2}};
    CHECK(sfl_batch_step_n_until(b, 2, prm, stop) == SFL_ERR_STATE && says("the torque recorder"), "step_n_until while full: %s", sfl_last_error());
    CHECK(events.empty() && b->d_members == members_before && b->member_slot == slot_before && info_is(b, sfl_batch_torque_info, 2, 2, 4, 1) && b->torque.on &&
              b->torque.d_records == buffer && sfl_batch_forces_pending(b, &pending, nullptr) == SFL_OK && pending == 1,
          "a refused call stages, launches and counts nothing, and leaves the recorder as it was");
    CHECK(sfl_batch_step_n(b, 1, DT, DX, 4, OMEGA) == SFL_OK && kinds() == "s" && info_is(b, sfl_batch_torque_info, 2, 2, 5, 1), "one step completes none: let through");
    // ---- set_bodies while a recorder is on: its own checks first, then the refusal, each with its message
    uint8_t labels[B * CELLS];
    for (int k = 0; k < B * CELLS; ++k) labels[k] = (uint8_t)(k % 4);
    CHECK(sfl_batch_set_bodies(b, labels, 0, 2) == SFL_ERR_INVALID && says("label 3 of cell (3, 0) of member 0 exceeds bodies = 2"), "the first offending cell: %s", sfl_last_error());
    CHECK(sfl_batch_set_bodies(b, labels, 0, 3) == SFL_ERR_STATE && says("sfl_batch_set_bodies: the torque recorder is on") && says("sfl_batch_torque_stop") && !says("loads recorder") &&
              !says("friction") && b->loads.d_labels == nullptr && b->loads.bodies == 1, "set_bodies while the torque is recorded: %s", sfl_last_error());
    CHECK(sfl_batch_set_bodies(b, nullptr, 0, 1) == SFL_ERR_STATE && says("the torque recorder is on"), "... going back too");
    CHECK(sfl_batch_friction_start(b, 2, 0, B, 2) == SFL_OK && sfl_batch_set_bodies(b, labels, 0, 3) == SFL_ERR_STATE && says("the friction recorder is on") && !says("torque"),
          "friction and torque on: the friction's message, as it was: %s", sfl_last_error());
    CHECK(sfl_batch_friction_stop(b) == SFL_OK && sfl_batch_torque_stop(b) == SFL_OK && b->torque_step == nullptr && b->torque.d_pivot2 != nullptr, "stop keeps the pivots");
    CHECK(sfl_batch_set_bodies(b, labels, 0, 3) == SFL_OK && b->torque.d_pivot2 == nullptr && b->torque.h_pivot2.empty(), "another number of bodies: the pivots go back to (0, 0): %s", sfl_last_error());
    CHECK(sfl_batch_set_bodies(b, nullptr, 0, 1) == SFL_OK, "labels off");
    // ---- with solids: loads, friction, then torque behind the step that is due; a restart keeps the buffer
    CHECK(sfl_batch_torque_start(b, 2, 1, 2, 2) == SFL_OK && sfl_batch_torque_start(b, 2, 1, 2, 2) == SFL_OK && info_is(b, sfl_batch_torque_info, 0, 2, 0, 1), "start twice: %s", sfl_last_error());
    buffer = b->torque.d_records;
    CHECK(sfl_batch_torque_start(b, 2, 1, 2, 1) == SFL_OK && b->torque.d_records == buffer && sfl_batch_torque_start(b, 2, 1, 2, 2) == SFL_OK && b->torque.d_records == buffer,
          "a restart that needs no more keeps the buffer");
    CHECK(sfl_batch_set_solids(b, MASK, 0) == SFL_OK && sfl_batch_loads_start(b, 2, 0, B, 2) == SFL_OK && sfl_batch_friction_start(b, 2, 0, B, 2) == SFL_OK, "solids, loads, friction: %s", sfl_last_error());
    CHECK(sfl_batch_set_body_pivots(b, each, 1, 1) == SFL_OK, "pivots per member");
    events.clear();
    CHECK(sfl_batch_step_n(b, 2, DT, DX, 4, OMEGA) == SFL_OK && kinds() == "SSLFT" && info_is(b, sfl_batch_torque_info, 1, 2, 2, 1) && info_is(b, sfl_batch_loads_info, 1, 2, 2, 1) &&
              info_is(b, sfl_batch_friction_info, 1, 2, 2, 1), "loads, friction, torque: %s", kinds().c_str());
    if (kinds() == "SSLFT") {
        const sfl::BatchTorqueSample &a = events[4].batch;
        CHECK((const void *)a.v == (const void *)b->vel && a.p == b->p && a.codes == b->solids.d_codes && a.code_stride == 0 && a.labels == nullptr && a.pivot2 == b->torque.d_pivot2 &&
                  a.pivot_stride == 2 && a.dim_x == X && a.dim_y == Y && a.first == 1 && a.count == 2 && a.bodies == 1 && a.out == static_cast<struct sfl_body_torque *>(buffer) + B,
              "what the sampler is handed: the fields the step left, the pivots' table and its stride");
    }
    CHECK(sfl_batch_step_n_each(b, 2, prm) == SFL_OK && kinds() == "SSLFTEELFT" && events[9].batch.out == static_cast<struct sfl_body_torque *>(buffer) + B + 2 &&
              (const void *)events[9].batch.v == (const void *)b->vel, "the second sample's slot: %s", kinds().c_str());
    CHECK(sfl_batch_torque_read(b, 0, 2, rec, 4 * REC) == SFL_OK && all_bytes(rec, 4 * REC, 0x6b), "the torque samples that were launched");
    CHECK(sfl_batch_loads_read(b, 0, 2, lrec, 2 * B * sizeof lrec[0]) == SFL_OK && all_bytes(lrec, 2 * B * sizeof lrec[0], 0x3c), "... the loads' own, in a buffer of their own");
    CHECK(sfl_batch_friction_read(b, 0, 2, frec, 2 * B * sizeof frec[0]) == SFL_OK && all_bytes(frec, 2 * B * sizeof frec[0], 0x5a), "... and the friction's");
    // all full: the loads' admission comes first, then the friction's, then the torque's
    CHECK(sfl_batch_step_n(b, 2, DT, DX, 4, OMEGA) == SFL_ERR_STATE && says("the loads recorder has room"), "all full: %s", sfl_last_error());
    CHECK(sfl_batch_loads_stop(b) == SFL_OK && sfl_batch_step_n(b, 2, DT, DX, 4, OMEGA) == SFL_ERR_STATE && says("the friction recorder has room"), "then the friction's: %s", sfl_last_error());
    CHECK(sfl_batch_friction_stop(b) == SFL_OK && sfl_batch_step_n(b, 2, DT, DX, 4, OMEGA) == SFL_ERR_STATE && says("the torque recorder has room"), "the torque's alone: %s", sfl_last_error());
    // the synchronous call beside the recorder: the room in front
    events.clear();
    CHECK(sfl_batch_torque(b, 2, 1, rec, REC) == SFL_OK && kinds() == "T" && events[0].batch.first == 2 && events[0].batch.count == 1 && events[0].batch.out == buffer &&
              b->torque.d_records == buffer && all_bytes(rec, REC, 0x6b), "torque beside the recorder: %s", sfl_last_error());
    // ---- labels: the loads' labels, strides and bodies reach the torque sampler; shared pivots have stride 0
    CHECK(sfl_batch_torque_stop(b) == SFL_OK && sfl_batch_set_bodies(b, labels, 1, 3) == SFL_OK, "labels per member: %s", sfl_last_error());
    const int32_t three[6] = {1, 1, 2, 2, 3, 3};
    CHECK(sfl_batch_set_body_pivots(b, three, 0, 3) == SFL_OK, "three shared pivots: %s", sfl_last_error());
    events.clear();
    CHECK(sfl_batch_torque(b, 1, 2, rec, 3 * 2 * REC) == SFL_OK && kinds() == "T" && events[0].batch.labels == b->loads.d_labels && events[0].batch.label_stride == (size_t)CELLS &&
              events[0].batch.code_stride == 0 && events[0].batch.pivot_stride == 0 && events[0].batch.pivot2 == b->torque.d_pivot2 && events[0].batch.bodies == 3 &&
              events[0].batch.first == 1 && b->torque.d_bytes == 3 * B * REC, "labels per member, mask shared: %s", sfl_last_error());
    CHECK(info_is(b, sfl_batch_torque_info, 0, 0, 0, 3), "info without a recorder: zeros and the bodies");
    CHECK(sfl_batch_set_body_pivots(b, nullptr, 0, 0) == SFL_OK && b->torque.d_pivot2 == nullptr && sfl_batch_set_bodies(b, nullptr, 0, 1) == SFL_OK, "pivots and labels off");
    // ---- a timeline replayed in one launch: no cut, the samples inside are zeros
    CHECK(sfl_batch_set_solids(b, nullptr, 0) == SFL_OK && sfl_batch_forget_forces(b) == SFL_OK && sfl_batch_torque_start(b, 1, 0, B, 4) == SFL_OK, "every step, no solids: %s", sfl_last_error());
    buffer = b->torque.d_records;
    memset(buffer, 0xff, b->torque.d_bytes);
    CHECK(sfl_batch_queue_forces_at(b, 0, ms, cells, vels, 1) == SFL_OK && sfl_batch_queue_forces_at(b, 2, ms + 1, cells + 2, vels + 2, 1) == SFL_OK, "a timeline");
    events.clear();
    CHECK(sfl_batch_step_n(b, 4, DT, DX, 4, OMEGA) == SFL_OK && kinds(false) == "p" && events[0].n == 4 && info_is(b, sfl_batch_torque_info, 4, 4, 4, 1), "the replay is not cut: %s", kinds().c_str());
    CHECK(sfl_batch_torque_read(b, 0, 4, rec, 4 * B * REC) == SFL_OK && all_bytes(rec, 4 * B * REC, 0), "its samples are zeros");
    // ---- stopped: the hook is gone, the buffer freed, the launch log the one of the null pointer
    CHECK(sfl_batch_torque_stop(b) == SFL_OK && b->torque_step == nullptr && !b->torque.on && b->torque.d_records == nullptr && info_is(b, sfl_batch_torque_info, 0, 0, 0, 1), "stop");
    CHECK(sfl_batch_torque_stop(b) == SFL_OK, "stop without a recorder");
    events.clear();
    CHECK(baseline() && kinds() == log0, "recorder off: the log of before (%s, %s)", kinds().c_str(), log0.c_str());
    // ---- a large batch has no solids: zeros and the pivots, and a recorder of the same
    events.clear();
    CHECK(sfl_batch_set_body_pivots(large, shared, 0, 1) == SFL_OK && sfl_batch_torque(large, 0, B, rec, B * REC) == SFL_OK && zeros_and_pivots(rec, B, 1, shared, 0, 0) &&
              sfl_batch_torque_start(large, 1, 0, B, 2) == SFL_OK && sfl_batch_step_n(large, 2, DT, DX, 4, OMEGA) == SFL_OK && kinds() == "sZsZ" &&
              info_is(large, sfl_batch_torque_info, 2, 2, 2, 1), "large: %s (%s)", kinds().c_str(), sfl_last_error());
    // ---- destroy with all three recorders on and pivots set
    CHECK(sfl_batch_set_body_pivots(b, each, 1, 1) == SFL_OK && sfl_batch_torque_start(b, 1, 0, B, 2) == SFL_OK && sfl_batch_friction_start(b, 1, 0, B, 2) == SFL_OK &&
              sfl_batch_loads_start(b, 1, 0, B, 2) == SFL_OK, "recorders to destroy");
    CHECK(sfl_batch_destroy(b) == SFL_OK && sfl_batch_destroy(large) == SFL_OK, "destroy");
    events.clear();
}

static void contexts()
{
    const int CX = 8, CY = 6, CC = CX * CY;
    sfl_context *c = nullptr, *slab = nullptr;
    CHECK(sfl_create(&c, 0, CX, CY) == SFL_OK && sfl_create_slab(&slab, 0, CX, 2 * CY, 0, 2) == SFL_OK && c && slab, "create: %s", sfl_last_error());
    if (!c || !slab) return;
    uint8_t mask[CC] = {}, labels[CC] = {};
    mask[2 * CX + 3] = mask[2 * CX + 4] = 1;
    labels[2 * CX + 3] = 1, labels[2 * CX + 4] = 2;
    struct sfl_body_torque rec[8];
    const int32_t one[2] = {5, -9}, two[4] = {1, 2, 3, 4};
    int32_t got[4];
    // ---- a slab: refused as from sfl_loads, the call's own checks first
    CHECK(sfl_torque(slab, rec, REC) == SFL_ERR_STATE && says("sfl_torque: whole-domain contexts only (slab 0/2): a slab has no solid cells and no torque"), "slab: %s", sfl_last_error());
    CHECK(sfl_torque_start(slab, 0, 1) == SFL_ERR_INVALID && sfl_torque_start(slab, 1, 1) == SFL_ERR_STATE && says("sfl_torque_start: whole-domain contexts only") && !slab->torque.on &&
              slab->torque_step == nullptr, "slab: %s", sfl_last_error());
    CHECK(sfl_torque_read(slab, 0, 0, rec, 0) == SFL_ERR_STATE && says("sfl_torque_read: whole-domain contexts only") && sfl_torque_stop(slab) == SFL_OK, "slab: read refused, stop let through");
    CHECK(sfl_set_body_pivots(slab, one, 1) == SFL_ERR_STATE && says("sfl_set_body_pivots: whole-domain contexts only") && sfl_set_body_pivots(slab, nullptr, 1) == SFL_OK, "slab: pivots refused, NULL let through");
    // ---- the unit's pointer is null; the fused boundaries of sfl_step_n on the tiled kernels
    CHECK(sfl_set_option(c, SFL_OPT_ADVECT_KERNEL, 2) == SFL_OK && sfl_set_option(c, SFL_OPT_SMALL_GRID, 0) == SFL_OK, "tiled, no one-launch step");
    const auto baseline = [&] { return sfl_step(c, DT, DX, 4, OMEGA) == SFL_OK && sfl_step_n(c, 3, DT, DX, 4, OMEGA) == SFL_OK; };
    events.clear();
    CHECK(c->torque_step == nullptr && baseline() && c->torque_step == nullptr, "baseline: %s", sfl_last_error());
    const std::string log0 = kinds();
    CHECK(log0 == "AAMM", "a step, then three with two seams: %s", log0.c_str());
    CHECK(sfl_torque(c, rec, REC) == SFL_OK && all_bytes(rec, REC, 0) && kinds() == log0 && c->torque.d_records == nullptr, "no solids: zeros, no launch");
    CHECK(sfl_torque(c, rec, 2 * REC) == SFL_ERR_INVALID && says("sfl_torque: the records of 1 bodies of 64 bytes each are 64 bytes, got 128") && !says("member"), "bytes: %s", sfl_last_error());
    CHECK(sfl_set_body_pivots(c, two, 2) == SFL_ERR_INVALID && says("sfl_set_body_pivots: bodies must be the 1 that sfl_bodies_info reports (got 2)"), "bodies: %s", sfl_last_error());
    CHECK(sfl_set_body_pivots(c, one, 1) == SFL_OK && sfl_body_pivots_download(c, got, 8) == SFL_OK && memcmp(got, one, 8) == 0, "a pivot: %s", sfl_last_error());
    CHECK(sfl_body_pivots_download(c, got, 16) == SFL_ERR_INVALID && says("sfl_body_pivots_download: the pivots of 1 bodies are 8 bytes, got 16"), "%s", sfl_last_error());
    // ---- the recorder without solids keeps the seams; its samples are zeros and the pivot
    CHECK(sfl_torque_start(c, 2, 2) == SFL_OK && c->torque_step && c->loads_step == nullptr && c->friction_step == nullptr && c->torque.d_bytes == 3 * REC, "start: %s", sfl_last_error());
    memset(c->torque.d_records, 0xff, c->torque.d_bytes);
    events.clear();
    CHECK(baseline() && kinds(false) == log0 && kinds() == "AAMZMZ" && info_is(c, sfl_torque_info, 2, 2, 4, 1), "recorder on, no solids: the same step launches, the seams uncut (%s)", kinds().c_str());
    CHECK(sfl_torque_read(c, 0, 2, rec, 2 * REC) == SFL_OK && zeros_and_pivots(rec, 2, 1, one, 0, 0), "two samples of zeros and the pivot");
    // ---- full: sfl_step_n and sfl_step are refused whole (admission points 4 and 5)
    events.clear();
    void *buffer = c->torque.d_records;
    CHECK(sfl_step_n(c, 2, DT, DX, -1, OMEGA) == SFL_ERR_INVALID && says("iters must be >= 0"), "iters first: %s", sfl_last_error());
    CHECK(sfl_step_n(c, 2, DT, DX, 4, OMEGA) == SFL_ERR_STATE && says("the torque recorder has room for 0 more samples (2 of 2 written) and 2 steps would complete 1") && says("sfl_torque_read") &&
              events.empty() && info_is(c, sfl_torque_info, 2, 2, 4, 1), "step_n while full: %s", sfl_last_error());
    CHECK(sfl_step_n(c, 1, DT, DX, 4, OMEGA) == SFL_OK && kinds() == "A" && info_is(c, sfl_torque_info, 2, 2, 5, 1), "one step completes none: %s", kinds().c_str());
    CHECK(sfl_step(c, DT, DX, 4, OMEGA) == SFL_ERR_STATE && says("the torque recorder has room for 0 more samples") && kinds() == "A" && info_is(c, sfl_torque_info, 2, 2, 5, 1) &&
              c->torque.on && c->torque.d_records == buffer, "step while full: refused whole, the recorder untouched: %s", sfl_last_error());
    // ---- set_bodies while the recorder is on
    CHECK(sfl_set_bodies(c, labels, 2) == SFL_ERR_STATE && says("sfl_set_bodies: the torque recorder is on") && says("sfl_torque_stop"), "set_bodies while recording: %s", sfl_last_error());
    CHECK(sfl_loads_start(c, 1, 1) == SFL_OK && sfl_set_bodies(c, labels, 2) == SFL_ERR_STATE && says("the loads recorder is on") && !says("torque") && sfl_loads_stop(c) == SFL_OK,
          "... and the loads' message first: %s", sfl_last_error());
    CHECK(sfl_torque_stop(c) == SFL_OK && c->torque_step == nullptr && c->torque.d_records == nullptr, "stop");
    // ---- labels and a mask: the sampler behind the history's passes, the loads' and the friction's, last
    CHECK(sfl_set_bodies(c, labels, 2) == SFL_OK && c->torque.d_pivot2 == nullptr && sfl_set_body_pivots(c, two, 2) == SFL_OK && sfl_set_solids(c, mask) == SFL_OK &&
              sfl_torque_start(c, 2, 2) == SFL_OK && sfl_friction_start(c, 2, 2) == SFL_OK && sfl_loads_start(c, 2, 2) == SFL_OK && sfl_history_start(c, 1, 8) == SFL_OK &&
              c->torque.d_bytes == (2 + 2 * 2) * REC, "mask, four recorders: %s", sfl_last_error());
    events.clear();
    CHECK(sfl_step_n(c, 2, DT, DX, 4, OMEGA) == SFL_OK && kinds() == "aDKGfaDKGfCXY" && info_is(c, sfl_torque_info, 1, 2, 2, 2), "with solids: %s", kinds().c_str());
    if (!events.empty() && events.back().kind == 'Y') {
        const sfl::ContextTorqueSample &a = events.back().context;
        CHECK((const void *)a.v == (const void *)c->vel && a.p == c->p && a.codes == c->solids.d_codes && a.labels == c->loads.d_labels && a.pivot2 == c->torque.d_pivot2 && a.dim_x == CX &&
                  a.dim_y == CY && a.bodies == 2 && a.out == static_cast<struct sfl_body_torque *>(c->torque.d_records) + 2, "what the sampler is handed");
    }
    CHECK(sfl_step(c, DT, DX, 4, OMEGA) == SFL_OK && sfl_step(c, DT, DX, 4, OMEGA) == SFL_OK && kinds() == "aDKGfaDKGfCXYaDKGfaDKGfCXY", "sfl_step: the same order: %s", kinds().c_str());
    events.clear();
    CHECK(sfl_torque(c, rec, 2 * REC) == SFL_OK && kinds() == "Y" && events[0].context.out == c->torque.d_records && all_bytes(rec, 2 * REC, 0x6b), "torque beside the recorder");
    CHECK(sfl_torque_read(c, 0, 2, rec, 4 * REC) == SFL_OK && all_bytes(rec, 4 * REC, 0x6b), "the samples");
    CHECK(sfl_torque_read(c, 0, 1, rec, REC) == SFL_ERR_INVALID && says("1 samples of 2 records of 64 bytes (1 context of 2 bodies) are 128 bytes, got 64"), "read: bytes: %s", sfl_last_error());
    // ---- recorder off: the log of the null pointer
    CHECK(sfl_history_stop(c) == SFL_OK && sfl_loads_stop(c) == SFL_OK && sfl_friction_stop(c) == SFL_OK && sfl_set_solids(c, nullptr) == SFL_OK && sfl_torque_stop(c) == SFL_OK &&
              c->torque_step == nullptr, "all off");
    events.clear();
    CHECK(baseline() && kinds() == log0, "recorder off: the log of before (%s)", kinds().c_str());
    CHECK(sfl_torque_start(c, 1, 2) == SFL_OK, "a recorder to destroy, the pivots still set");
    CHECK(sfl_destroy(c) == SFL_OK && sfl_destroy(slab) == SFL_OK, "destroy");
    events.clear();
}

// torque_face.h face by face, through two files
static int run_faces(const char *in_path, const char *out_path)
{
    FILE *in = fopen(in_path, "rb"), *out = fopen(out_path, "wb");
    if (!in || !out) return 2;
    long n = 0;
    int64_t r[9];
    while (fread(r, 8, 9, in) == 9) {
        using namespace sfl::torque_face;
        const int dir = (int)r[2];
        const Arms a = arms_of((int)r[0], (int)r[1], dir, (int32_t)r[3], (int32_t)r[4]);
        const int64_t w[8] = {a.rx2, a.ry2, (int64_t)longest(a), pressure_moment(a, dir, r[5]), friction_moment(a, dir, r[6]),
                              bit_length((uint32_t)r[7]), bit_length((uint32_t)r[8]), shift_of((uint32_t)r[7], (uint32_t)r[8])};
        if (fwrite(w, 8, 8, out) != 8) return 4;
        ++n;
    }
    fclose(in);
    if (fclose(out)) return 4;
    printf("%ld faces through torque_face.h\n", n);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 3) return run_faces(argv[1], argv[2]);
    refusals_without_handles();
    batches();
    contexts();
    const long left = fake_hip_live_allocations();
    printf("torque driver: %d failed checks, %ld allocations left\n", failures, left);
    return failures || left ? 1 : 0;
}
