// means_driver.cpp -- TEST HARNESS (tests/cpp, `make -f means.mk`; tests/test_means.py): the HOST side of the averages
// (csrc/means.cpp) and of its hooks in the step calls (csrc/batch.cpp, csrc/slab_step.cpp), run on a box without a GPU: the
// host units over the runtime that lives on the host (fake_hip.cpp) and kernels that do nothing (launch_stubs_ok.cpp).  The
// launchers of the batches, of the solids, of the histories, of the loads, of the friction and of the averages are stubs of
// THIS file that keep ONE log in the order of the calls, which is the order of the stream.  What is checked: the argument
// refusals, each with the call's own name; the order history, loads, friction, averages behind a step; a batch's one-launch
// replay cut at the steps whose sample is due and NOT cut with every == 0; sfl_step_n without its fused boundaries only while
// the hook is set; the number of planes and their bytes for every mask, the padded member stride and what the sampler is
// handed; a restart zeroing the planes; steps counted across calls; the downloads, dense whatever the padding; stop and
// destroy freeing the planes; with no averages on the launch log of every step call identical to the one made while the
// unit's pointer was still null.  Exit status 0 and "0 failed checks".
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../esp32-fluid-simulation_amd/csrc/batch_state.h"
#include "../../esp32-fluid-simulation_amd/csrc/friction_kernels.h"
#include "../../esp32-fluid-simulation_amd/csrc/history_kernels.h"
#include "../../esp32-fluid-simulation_amd/csrc/load_kernels.h"
#include "../../esp32-fluid-simulation_amd/csrc/mean_kernels.h"
#include "../../esp32-fluid-simulation_amd/csrc/solid_kernels.h"
#include "../../esp32-fluid-simulation_amd/csrc/until_kernels.h"
#include "../../esp32-fluid-simulation_amd/csrc/view_kernels.h"
#include "../../include/sfl.h"

extern "C" long fake_hip_live_allocations();

// (the host runtime of fake_hip.cpp has no pitched copy: the one the downloads of a padded plane make)
hipError_t hipMemcpy2DAsync(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t height, hipMemcpyKind, hipStream_t)
{
    for (size_t r = 0; r < height; ++r) memmove(static_cast<char *>(dst) + r * dpitch, static_cast<const char *>(src) + r * spitch, width);
    return hipSuccess;
}

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
// 'C' a context's; 'F' a batch's friction sample, 'X' a context's; 'N' a sample of the averages
struct Event {
    char kind;
    int n;
    sfl::MeanSample mean;
};
static std::vector<Event> events;
static hipError_t note(char kind, int n = 0)
{
    events.push_back({kind, n, {}});
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
// the sample of the averages: every cell of every live plane of every recorded member counts the samples it has seen, the
// member's last cell a thousand at a time -- a plane that was not zeroed, a wrong stride and a wrong plane all show
hipError_t launch_mean_sample(hipStream_t, const MeanSample &a)
{
    for (int k = 0; k < SFL_MEAN_PLANES; ++k) {
        if (!a.plane[k]) continue;
        for (int m = 0; m < a.count; ++m)
            for (size_t c = 0; c < a.cells; ++c) {
                const double add = (c + 1 == a.cells ? 1000.0 : 1.0) + k;
                if (k >= SFL_MEAN_PLANE_R)
                    reinterpret_cast<uint64_t *>(a.plane[k])[(size_t)m * a.member_stride + c] += (uint64_t)add;
                else
                    a.plane[k][(size_t)m * a.member_stride + c] += add;
            }
    }
    events.push_back({'N', a.count, a});
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

static const int B = 4, X = 3, Y = 3, CELLS = X * Y;   // an odd number of cells: the planes are padded to 10 values per member

template <class H>
static bool info_is(H *x, int (*info)(H *, int *, int *, int64_t *, int64_t *), int what, int every, int64_t samples, int64_t steps)
{
    int w = -1, e = -1;
    int64_t s = -1, t = -1;
    const bool ok = info(x, &w, &e, &s, &t) == SFL_OK && w == what && e == every && s == samples && t == steps;
    if (!ok) fprintf(stderr, "  info: what %d, every %d, %lld samples, %lld steps\n", w, e, (long long)s, (long long)t);
    return ok;
}

static void refusals_without_handles()
{
    double host[4];
    int w = 5;
    CHECK(sfl_batch_mean_start(nullptr, 0, 1, 0, 1) == SFL_ERR_INVALID && says("sfl_batch_mean_start: what must be a mask of SFL_MEAN_* groups, 1..15 (got 0)"), "%s", sfl_last_error());
    CHECK(sfl_batch_mean_start(nullptr, 16, 1, 0, 1) == SFL_ERR_INVALID && says("1..15 (got 16)"), "%s", sfl_last_error());
    CHECK(sfl_batch_mean_start(nullptr, 1, -1, 0, 1) == SFL_ERR_INVALID && says("sfl_batch_mean_start: every must be >= 0 (got -1)"), "%s", sfl_last_error());
    CHECK(sfl_batch_mean_start(nullptr, 1, 0, 0, 0) == SFL_ERR_INVALID && says("sfl_batch_mean_start: count must be >= 1 (got 0)"), "%s", sfl_last_error());
    CHECK(sfl_batch_mean_start(nullptr, 1, 0, 0, 1) == SFL_ERR_INVALID && says("sfl_batch_mean_start: batch is NULL"), "%s", sfl_last_error());
    CHECK(sfl_batch_mean_stop(nullptr) == SFL_ERR_INVALID && says("sfl_batch_mean_stop: batch is NULL"), "%s", sfl_last_error());
    CHECK(sfl_batch_mean_sample(nullptr) == SFL_ERR_INVALID && says("sfl_batch_mean_sample: batch is NULL"), "%s", sfl_last_error());
    CHECK(sfl_batch_mean_info(nullptr, &w, &w, nullptr, nullptr) == SFL_ERR_INVALID && says("sfl_batch_mean_info: batch is NULL") && w == 5, "%s", sfl_last_error());
    CHECK(sfl_batch_mean_download(nullptr, 10, 0, 1, host, 8) == SFL_ERR_INVALID && says("sfl_batch_mean_download: plane must be one of SFL_MEAN_PLANE_*, 0..9 (got 10)"), "%s", sfl_last_error());
    CHECK(sfl_batch_mean_download(nullptr, 0, 0, 0, host, 8) == SFL_ERR_INVALID && says("sfl_batch_mean_download: members must be >= 1 (got 0)"), "%s", sfl_last_error());
    CHECK(sfl_batch_mean_download(nullptr, 0, 0, 1, host, 8) == SFL_ERR_INVALID && says("sfl_batch_mean_download: batch is NULL"), "%s", sfl_last_error());
    CHECK(sfl_mean_start(nullptr, -2, 1) == SFL_ERR_INVALID && says("sfl_mean_start: what must be a mask"), "%s", sfl_last_error());
    CHECK(sfl_mean_start(nullptr, 15, -3) == SFL_ERR_INVALID && says("sfl_mean_start: every must be >= 0 (got -3)"), "%s", sfl_last_error());
    CHECK(sfl_mean_start(nullptr, 15, 0) == SFL_ERR_INVALID && says("sfl_mean_start: ctx is NULL"), "%s", sfl_last_error());
    CHECK(sfl_mean_stop(nullptr) == SFL_ERR_INVALID && says("sfl_mean_stop: ctx is NULL"), "%s", sfl_last_error());
    CHECK(sfl_mean_sample(nullptr) == SFL_ERR_INVALID && says("sfl_mean_sample: ctx is NULL"), "%s", sfl_last_error());
    CHECK(sfl_mean_info(nullptr, nullptr, nullptr, nullptr, nullptr) == SFL_ERR_INVALID && says("sfl_mean_info: ctx is NULL"), "%s", sfl_last_error());
    CHECK(sfl_mean_download(nullptr, -1, host, 8) == SFL_ERR_INVALID && says("sfl_mean_download: plane must be one of SFL_MEAN_PLANE_*, 0..9 (got -1)"), "%s", sfl_last_error());
    CHECK(sfl_mean_download(nullptr, 9, host, 8) == SFL_ERR_INVALID && says("sfl_mean_download: ctx is NULL"), "%s", sfl_last_error());
    CHECK(events.empty(), "a refused call launches nothing");
}

static void batches()
{
    sfl_batch *b = nullptr, *large = nullptr;
    CHECK(sfl_batch_create(&b, 0, X, Y, B) == SFL_OK && sfl_batch_create_large(&large, 0, X, Y, B) == SFL_OK && b && large, "create: %s", sfl_last_error());
    if (!b || !large) return;
    sfl_member_params prm[B];
    for (int m = 0; m < B; ++m) prm[m] = {DT * (m + 1), DX, OMEGA, 3 + m};
    sfl_member_stop stop[B] = {{-1.0f, 2}, {-1.0f, 2}, {-1.0f, 2}, {-1.0f, 2}};
    const auto baseline = [&] {
        return sfl_batch_step_n(b, 2, DT, DX, 4, OMEGA) == SFL_OK && sfl_batch_step_n_each(b, 1, prm) == SFL_OK && sfl_batch_step_n_until(b, 1, prm, stop) == SFL_OK;
    };
    double host[B * CELLS];
    uint64_t dye[B * CELLS];
    // ---- the unit's pointer is null: the log to compare with
    events.clear();
    CHECK(b->mean_step == nullptr && baseline() && kinds() == "sseu" && b->mean_step == nullptr, "baseline: %s", kinds().c_str());
    const std::string log0 = kinds();
    CHECK(info_is(b, sfl_batch_mean_info, 0, 0, 0, 0), "info without averages: zeros");
    CHECK(sfl_batch_mean_sample(b) == SFL_ERR_STATE && says("sfl_batch_mean_sample: no averages to add to: call sfl_mean_start (sfl_batch_mean_start) first"), "sample without: %s", sfl_last_error());
    CHECK(sfl_batch_mean_download(b, 0, 0, 1, host, CELLS * 8) == SFL_ERR_STATE && says("sfl_batch_mean_download: no averages to download"), "download without: %s", sfl_last_error());
    CHECK(sfl_batch_mean_stop(b) == SFL_OK, "stop without averages");
    // ---- planes and bytes for every mask; the stride is the member's cells rounded up to an even number
    const int planes_of[16] = {0, 2, 3, 5, 2, 4, 5, 7, 3, 5, 6, 8, 5, 7, 8, 10};
    const long live0 = fake_hip_live_allocations();
    for (int what = 1; what <= 15; ++what) {
        CHECK(sfl_batch_mean_start(b, what, 0, 1, 2) == SFL_OK && b->means.on && b->means.what == (unsigned)what && b->means.member_stride == 10 &&
                  b->means.d_bytes == (size_t)planes_of[what] * 2 * 10 * 8 && b->mean_step == nullptr && all_bytes(b->means.d_planes, b->means.d_bytes, 0),
              "mask %d: %zu bytes: %s", what, b->means.d_bytes, sfl_last_error());
        CHECK(fake_hip_live_allocations() == live0 + 1, "a start while on frees the planes it replaces");
        events.clear();
        CHECK(sfl_batch_mean_sample(b) == SFL_OK && kinds() == "N", "a sample: %s", sfl_last_error());
        if (kinds() != "N") continue;
        const sfl::MeanSample &a = events[0].mean;
        int live = 0;
        for (int k = 0; k < SFL_MEAN_PLANES; ++k) {
            const bool want = (k < 2 ? what & 1 : k < 5 ? what & 2 : k < 7 ? what & 4 : what & 8) != 0;
            CHECK((a.plane[k] != nullptr) == want, "mask %d plane %d", what, k);
            if (a.plane[k]) CHECK(a.plane[k] == static_cast<double *>(b->means.d_planes) + (size_t)live++ * 2 * 10, "mask %d plane %d: the live planes in the order of their ids", what, k);
        }
        CHECK((const void *)a.v == (const void *)b->vel && (const void *)a.p == (const void *)b->p && (const void *)a.dye == (const void *)b->col && a.cells == (size_t)CELLS &&
                  a.member_stride == 10 && a.first == 1 && a.count == 2 && a.what == (unsigned)what, "what the sampler is handed: the fields held, the recorded range");
    }
    // ---- range and argument checks with a handle
    CHECK(sfl_batch_mean_start(b, 1, 0, 3, 2) == SFL_ERR_INVALID && says("sfl_batch_mean_start: members [3, 3 + 2) are not inside the batch's [0, 4)") && b->means.on && b->means.what == 15,
          "a refused start leaves the averages as they were: %s", sfl_last_error());
    // ---- every == 0: no hook, nothing behind the steps, the replay uncut; manual samples only
    const int ms[2] = {0, 2}, cells[4] = {0, 0, 1, 0};
    const float vels[4] = {1, 0, 0, 1};
    CHECK(sfl_batch_mean_start(b, SFL_MEAN_VELOCITY | SFL_MEAN_DYE, 0, 1, 2) == SFL_OK && b->mean_step == nullptr, "every 0: %s", sfl_last_error());
    events.clear();
    CHECK(baseline() && kinds() == log0 && info_is(b, sfl_batch_mean_info, 9, 0, 0, 0), "every 0: the log of the null pointer, no step counted (%s)", kinds().c_str());
    CHECK(sfl_batch_queue_forces_at(b, 0, ms, cells, vels, 1) == SFL_OK && sfl_batch_queue_forces_at(b, 2, ms + 1, cells + 2, vels + 2, 1) == SFL_OK, "a timeline");
    events.clear();
    CHECK(sfl_batch_step_n(b, 4, DT, DX, 4, OMEGA) == SFL_OK && kinds() == "p" && events[0].n == 4, "every 0: the replay is not cut: %s", kinds().c_str());
    CHECK(sfl_batch_mean_sample(b) == SFL_OK && sfl_batch_mean_sample(b) == SFL_OK && info_is(b, sfl_batch_mean_info, 9, 0, 2, 0), "two manual samples");
    // the downloads: dense whatever the padding, members in order, the dye planes as integers
    memset(host, 0xff, sizeof host);
    CHECK(sfl_batch_mean_download(b, SFL_MEAN_PLANE_V, 1, 2, host, 2 * CELLS * 8) == SFL_OK, "download: %s", sfl_last_error());
    bool dense = true;
    for (int m = 0; m < 2; ++m)
        for (int c = 0; c < CELLS; ++c) dense &= host[m * CELLS + c] == 2 * ((c + 1 == CELLS ? 1000.0 : 1.0) + SFL_MEAN_PLANE_V);
    CHECK(dense && all_bytes(host + 2 * CELLS, 8, 0xff), "two members of 9 values each, packed");
    CHECK(sfl_batch_mean_download(b, SFL_MEAN_PLANE_B, 2, 1, dye, CELLS * 8) == SFL_OK && dye[0] == 2 * (1 + 9) && dye[CELLS - 1] == 2 * (1000 + 9), "a dye plane of the second recorded member");
    CHECK(sfl_batch_mean_download(b, SFL_MEAN_PLANE_P, 1, 2, host, 2 * CELLS * 8) == SFL_ERR_INVALID && says("sfl_batch_mean_download: plane 5 belongs to group 4, which is not in the mask 9"),
          "a plane outside the mask: %s", sfl_last_error());
    CHECK(sfl_batch_mean_download(b, SFL_MEAN_PLANE_U, 1, 2, host, 2 * CELLS * 8 + 8) == SFL_ERR_INVALID && says("a plane of 2 members of 9 values of 8 bytes is 144 bytes, got 152"),
          "bytes: %s", sfl_last_error());
    CHECK(sfl_batch_mean_download(b, SFL_MEAN_PLANE_U, 0, 2, host, 2 * CELLS * 8) == SFL_ERR_INVALID && says("members [0, 0 + 2) are not inside the recorded [1, 1 + 2)"), "range: %s", sfl_last_error());
    CHECK(sfl_batch_mean_download(b, SFL_MEAN_PLANE_U, 2, 2, host, 2 * CELLS * 8) == SFL_ERR_INVALID && says("members [2, 2 + 2) are not inside the recorded [1, 1 + 2)"), "range: %s", sfl_last_error());
    CHECK(sfl_batch_mean_download(b, SFL_MEAN_PLANE_U, 1, 1, nullptr, CELLS * 8) == SFL_ERR_INVALID && says("sfl_batch_mean_download: host is NULL"), "host: %s", sfl_last_error());
    // ---- a restart begins anew from zero
    CHECK(sfl_batch_mean_start(b, SFL_MEAN_VELOCITY, 3, 0, B) == SFL_OK && b->mean_step != nullptr && info_is(b, sfl_batch_mean_info, 1, 3, 0, 0) &&
              all_bytes(b->means.d_planes, b->means.d_bytes, 0) && b->means.d_bytes == (size_t)2 * B * 10 * 8, "restart: %s", sfl_last_error());
    // ---- every 3: steps counted across calls and across the three kinds of step call; a sample after steps 3 and 6
    events.clear();
    CHECK(baseline() && kinds() == "sseNu" && info_is(b, sfl_batch_mean_info, 1, 3, 1, 4), "four steps: %s", kinds().c_str());
    CHECK(sfl_batch_step_n(b, 3, DT, DX, 4, OMEGA) == SFL_OK && kinds() == "sseNussNs" && info_is(b, sfl_batch_mean_info, 1, 3, 2, 7), "... and three more: %s", kinds().c_str());
    CHECK(sfl_batch_mean_sample(b) == SFL_OK && info_is(b, sfl_batch_mean_info, 1, 3, 3, 7), "a manual sample counts as a sample, not as a step");
    // ---- a timeline: the replay is cut at the steps whose sample is due (8 steps from step 7: due after 9, 12, 15)
    CHECK(sfl_batch_queue_forces_at(b, 0, ms, cells, vels, 1) == SFL_OK && sfl_batch_queue_forces_at(b, 5, ms + 1, cells + 2, vels + 2, 1) == SFL_OK, "a timeline");
    events.clear();
    CHECK(sfl_batch_step_n(b, 8, DT, DX, 4, OMEGA) == SFL_OK && kinds() == "pNpNpN" && events[0].n == 2 && events[2].n == 3 && events[4].n == 3 && info_is(b, sfl_batch_mean_info, 1, 3, 6, 15),
          "the replay cut at the due steps: %s", kinds().c_str());
    // ... and with a history beside it at either's: history in front of the averages
    CHECK(sfl_batch_history_start(b, 2, 0, B, 8) == SFL_OK, "a history: %s", sfl_last_error());
    CHECK(sfl_batch_queue_forces_at(b, 0, ms, cells, vels, 1) == SFL_OK && sfl_batch_queue_forces_at(b, 3, ms + 1, cells + 2, vels + 2, 1) == SFL_OK, "a timeline");
    events.clear();
    CHECK(sfl_batch_step_n(b, 6, DT, DX, 4, OMEGA) == SFL_OK && kinds() == "pHpNpHpHN" && info_is(b, sfl_batch_mean_info, 1, 3, 8, 21), "history (2, 4, 6) and averages (18, 21): %s", kinds().c_str());
    events.clear();
    CHECK(sfl_batch_step_n(b, 3, DT, DX, 4, OMEGA) == SFL_OK && kinds() == "ssHsN" && sfl_batch_history_stop(b) == SFL_OK, "step by step: %s", kinds().c_str());
    // ---- loads and friction in front of the averages (no solids: their samples are zero-fills that launch nothing)
    CHECK(sfl_batch_loads_start(b, 1, 0, B, 4) == SFL_OK && sfl_batch_friction_start(b, 1, 0, B, 4) == SFL_OK && sfl_batch_mean_start(b, 15, 1, 0, B) == SFL_OK, "all on: %s", sfl_last_error());
    const uint8_t mask[CELLS] = {0, 0, 0, 0, 1, 0, 0, 0, 0};
    CHECK(sfl_batch_set_solids(b, mask, 0) == SFL_OK, "solids: %s", sfl_last_error());
    events.clear();
    CHECK(sfl_batch_step_n(b, 2, DT, DX, 4, OMEGA) == SFL_OK && kinds() == "SLFNSLFN", "loads, friction, averages behind every step: %s", kinds().c_str());
    CHECK(sfl_batch_loads_stop(b) == SFL_OK && sfl_batch_friction_stop(b) == SFL_OK && sfl_batch_set_solids(b, nullptr, 0) == SFL_OK, "off again");
    // ---- stopped: the hook is gone, the planes freed, the launch log the one of the null pointer
    const long live1 = fake_hip_live_allocations();   // (the timelines and the recorders above have made allocations that stay)
    CHECK(sfl_batch_mean_stop(b) == SFL_OK && b->mean_step == nullptr && !b->means.on && b->means.d_planes == nullptr && fake_hip_live_allocations() == live1 - 1 &&
              info_is(b, sfl_batch_mean_info, 0, 0, 0, 0), "stop");
    events.clear();
    CHECK(baseline() && kinds() == log0, "averages off: the log of before (%s, %s)", kinds().c_str(), log0.c_str());
    // ---- a large batch: the same calls
    events.clear();
    CHECK(sfl_batch_mean_start(large, SFL_MEAN_PRESSURE, 2, 0, B) == SFL_OK && sfl_batch_step_n(large, 4, DT, DX, 4, OMEGA) == SFL_OK && kinds() == "ssNssN" &&
              info_is(large, sfl_batch_mean_info, 4, 2, 2, 4), "large: %s (%s)", kinds().c_str(), sfl_last_error());
    // ---- destroy with averages on
    CHECK(sfl_batch_mean_start(b, 15, 1, 0, B) == SFL_OK, "averages to destroy");
    CHECK(sfl_batch_destroy(b) == SFL_OK && sfl_batch_destroy(large) == SFL_OK, "destroy");
    events.clear();
}

static void contexts()
{
    const int CX = 9, CY = 7, CC = CX * CY;   // 63 cells: a stride of 64
    sfl_context *c = nullptr, *slab = nullptr;
    CHECK(sfl_create(&c, 0, CX, CY) == SFL_OK && sfl_create_slab(&slab, 0, CX, 2 * CY, 0, 2) == SFL_OK && c && slab, "create: %s", sfl_last_error());
    if (!c || !slab) return;
    double host[CC];
    // ---- a slab: refused, the call's own checks first
    CHECK(sfl_mean_start(slab, 0, 1) == SFL_ERR_INVALID && sfl_mean_start(slab, 1, 1) == SFL_ERR_STATE && says("sfl_mean_start: whole-domain contexts only (slab 0/2)") && !slab->means.on &&
              slab->mean_step == nullptr, "slab: %s", sfl_last_error());
    CHECK(sfl_mean_sample(slab) == SFL_ERR_STATE && says("sfl_mean_sample: whole-domain contexts only"), "slab: %s", sfl_last_error());
    CHECK(sfl_mean_download(slab, 0, host, 8) == SFL_ERR_STATE && says("sfl_mean_download: whole-domain contexts only") && sfl_mean_stop(slab) == SFL_OK &&
              info_is(slab, sfl_mean_info, 0, 0, 0, 0), "slab: download refused, stop and info let through");
    // ---- the unit's pointer is null; the fused boundaries of sfl_step_n on the tiled kernels
    CHECK(sfl_set_option(c, SFL_OPT_ADVECT_KERNEL, 2) == SFL_OK && sfl_set_option(c, SFL_OPT_SMALL_GRID, 0) == SFL_OK, "tiled, no one-launch step");
    const auto baseline = [&] { return sfl_step(c, DT, DX, 4, OMEGA) == SFL_OK && sfl_step_n(c, 3, DT, DX, 4, OMEGA) == SFL_OK; };
    events.clear();
    CHECK(c->mean_step == nullptr && baseline() && c->mean_step == nullptr, "baseline: %s", sfl_last_error());
    const std::string log0 = kinds();
    CHECK(log0 == "AAMM", "a step, then three with two seams: %s", log0.c_str());
    const long live0 = fake_hip_live_allocations();
    // ---- every == 0: the seams stay
    CHECK(sfl_mean_start(c, 15, 0) == SFL_OK && c->mean_step == nullptr && c->means.member_stride == 64 && c->means.d_bytes == (size_t)10 * 64 * 8 && c->means.count == 1 &&
              fake_hip_live_allocations() == live0 + 1, "every 0: %s", sfl_last_error());
    events.clear();
    CHECK(baseline() && kinds() == log0 && info_is(c, sfl_mean_info, 15, 0, 0, 0), "every 0: fused as before (%s)", kinds().c_str());
    CHECK(sfl_mean_sample(c) == SFL_OK && kinds() == log0 + "N" && info_is(c, sfl_mean_info, 15, 0, 1, 0), "a manual sample: %s", sfl_last_error());
    if (events.back().kind == 'N') {
        const sfl::MeanSample &a = events.back().mean;
        CHECK((const void *)a.v == (const void *)c->vel && (const void *)a.p == (const void *)c->p && (const void *)a.dye == (const void *)c->col && a.cells == (size_t)CC &&
                  a.member_stride == 64 && a.first == 0 && a.count == 1 && a.what == 15 && a.plane[9] == static_cast<double *>(c->means.d_planes) + 9 * 64, "what the sampler is handed");
    }
    CHECK(sfl_mean_download(c, SFL_MEAN_PLANE_PP, host, CC * 8) == SFL_OK && host[0] == 1.0 + 6 && host[CC - 1] == 1000.0 + 6, "download: %s", sfl_last_error());
    CHECK(sfl_mean_download(c, SFL_MEAN_PLANE_PP, host, CC * 8 - 8) == SFL_ERR_INVALID && says("sfl_mean_download: a plane of 63 values of 8 bytes is 504 bytes, got 496") && !says("member"),
          "bytes: %s", sfl_last_error());
    // ---- every >= 1: sfl_step_n runs without its fused boundaries, every step as sfl_step runs it; steps count across calls
    CHECK(sfl_mean_start(c, SFL_MEAN_STRESS, 2) == SFL_OK && c->mean_step != nullptr && c->means.d_bytes == (size_t)3 * 64 * 8 && all_bytes(c->means.d_planes, c->means.d_bytes, 0) &&
              fake_hip_live_allocations() == live0 + 1, "restart: %s", sfl_last_error());
    events.clear();
    CHECK(baseline() && kinds() == "AANAAN" && info_is(c, sfl_mean_info, 2, 2, 2, 4), "the hook set: unfused, a sample after steps 2 and 4 (%s)", kinds().c_str());
    CHECK(sfl_mean_download(c, SFL_MEAN_PLANE_U, host, CC * 8) == SFL_ERR_INVALID && says("sfl_mean_download: plane 0 belongs to group 1, which is not in the mask 2"), "mask: %s", sfl_last_error());
    // ---- a mask, labels and every recorder: history, loads, friction, averages
    uint8_t mask[CC] = {};
    mask[2 * CX + 3] = 1;
    CHECK(sfl_set_solids(c, mask) == SFL_OK && sfl_history_start(c, 1, 8) == SFL_OK && sfl_loads_start(c, 2, 2) == SFL_OK && sfl_friction_start(c, 2, 2) == SFL_OK, "recorders: %s", sfl_last_error());
    events.clear();
    CHECK(sfl_step_n(c, 2, DT, DX, 4, OMEGA) == SFL_OK && kinds() == "aDKGfaDKGfCXN" && info_is(c, sfl_mean_info, 2, 2, 3, 6), "with solids: %s", kinds().c_str());
    CHECK(sfl_step(c, DT, DX, 4, OMEGA) == SFL_OK && sfl_step(c, DT, DX, 4, OMEGA) == SFL_OK && kinds() == "aDKGfaDKGfCXNaDKGfaDKGfCXN", "sfl_step: the same order: %s", kinds().c_str());
    CHECK(sfl_history_stop(c) == SFL_OK && sfl_loads_stop(c) == SFL_OK && sfl_friction_stop(c) == SFL_OK && sfl_set_solids(c, nullptr) == SFL_OK, "recorders off");
    // ---- stop: the hook gone, the planes freed, fused again
    CHECK(sfl_mean_stop(c) == SFL_OK && c->mean_step == nullptr && c->means.d_planes == nullptr && fake_hip_live_allocations() == live0 && info_is(c, sfl_mean_info, 0, 0, 0, 0), "stop");
    CHECK(sfl_mean_download(c, SFL_MEAN_PLANE_UU, host, CC * 8) == SFL_ERR_STATE && says("sfl_mean_download: no averages to download"), "download after stop: %s", sfl_last_error());
    events.clear();
    CHECK(baseline() && kinds() == log0, "averages off: the log of before (%s)", kinds().c_str());
    CHECK(sfl_mean_start(c, 15, 1) == SFL_OK, "averages to destroy");
    CHECK(sfl_destroy(c) == SFL_OK && sfl_destroy(slab) == SFL_OK, "destroy");
    events.clear();
}

int main()
{
    refusals_without_handles();
    batches();
    contexts();
    const long left = fake_hip_live_allocations();
    printf("means driver: %d failed checks, %ld allocations left\n", failures, left);
    return failures || left ? 1 : 0;
}
