// solids_driver.cpp -- TEST HARNESS (tests/cpp, `make -f solids.mk`; tests/test_solids.py): the HOST side of the solids
// (csrc/solids.cpp) and of its hooks in the step, solve and statistics calls (csrc/batch.cpp), in the history's start
// (csrc/history.cpp) and in the views (csrc/views.cpp), run on a box without a GPU: the host units of the batches over the
// runtime that lives on the host (fake_hip.cpp) and kernels that do nothing (launch_stubs_ok.cpp).  Every launcher of
// csrc/batch.h, the statistics' and the views' are stubs of THIS file that keep ONE log in the order of the calls, which is the
// order of the stream.  What is checked: the code bytes the device is handed for a hand-written mask; which launcher each call
// picks with and without solids, and with which member stride; that clearing the solids restores the old launchers; that a
// timeline replay falls back to a launch per step; the admission order -- a call's own argument checks, then the state
// refusals, each with its message, then (and only then) anything staged or launched; download and info; destroy with solids set
// leaves no allocation.  Exit status 0 and "0 failed checks".
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../esp32-fluid-simulation_amd/csrc/batch_state.h"
#include "../../esp32-fluid-simulation_amd/csrc/history_kernels.h"
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
struct Event {
    char kind;   // 's' 'e' 'u' a plain step (uniform, each, until), 'p' a replay, 'v' 'w' 'x' a plain solve (uniform, each, until);
                 // 'S' 'E' 'V' 'W' the same by the solids' rule; 'f' the plain statistics, 'D' the solids' velocity pass;
                 // 'H' a history's sample, 'c' a view's scalars
    int n;       // a replay: its steps; 'f': what; 'c': what
    sfl::BatchSolids solids;
};
static std::vector<Event> events;
static hipError_t note(char kind, int n = 0, sfl::BatchSolids s = {nullptr, 0})
{
    events.push_back({kind, n, s});
    return hipSuccess;
}

namespace sfl {
bool small_grid_fits(int dim_x, int dim_y)   // (the real rule of small_grid.hip; launch_stubs_ok.cpp's answer is "no")
{
    return dim_x >= 2 && dim_y >= 2 && (long long)dim_x * dim_y <= kSmallGridMaxCells &&
           (long long)dim_y * ((dim_x + 1) / 2) <= kSmallGridMaxCells / 2;
}
hipError_t launch_batch_step(hipStream_t, const BatchStep &, int) { return note('s'); }
hipError_t launch_batch_step_each(hipStream_t, const BatchStep &, int, const BatchMember *, float *) { return note('e'); }
hipError_t launch_batch_step_until(hipStream_t, const BatchStep &, int, const BatchMember *, const BatchStop *, float *, int *, bool) { return note('u'); }
hipError_t launch_batch_large_step(hipStream_t, const BatchStep &, int) { return note('s'); }
hipError_t launch_batch_large_step_each(hipStream_t, const BatchStep &, int, const BatchMember *, float *) { return note('e'); }
hipError_t launch_batch_large_step_until(hipStream_t, const BatchStep &, int, const BatchMember *, const BatchStop *, float *, int *, bool) { return note('u'); }
hipError_t launch_batch_play(hipStream_t, const BatchPlay &a, int, const BatchMember *, float *) { return note('p', a.steps); }
hipError_t launch_batch_solve(hipStream_t, float *, const float *, int, int, int, int, SorParams) { return note('v'); }
hipError_t launch_batch_solve_each(hipStream_t, float *, const float *, int, int, int, const BatchMember *, float *) { return note('w'); }
hipError_t launch_batch_solve_until(hipStream_t, float *, const float *, int, int, int, const BatchMember *, const BatchStop *, float *, int *) { return note('x'); }
hipError_t launch_batch_large_solve(hipStream_t, float *, const float *, int, int, int, int, SorParams) { return note('v'); }
hipError_t launch_batch_large_solve_each(hipStream_t, float *, const float *, int, int, int, const BatchMember *, float *) { return note('w'); }
hipError_t launch_batch_large_solve_until(hipStream_t, float *, const float *, int, int, int, const BatchMember *, const BatchStop *, float *, int *) { return note('x'); }
hipError_t launch_batch_solid_step(hipStream_t, const BatchStep &, const BatchSolids &s, int) { return note('S', 0, s); }
hipError_t launch_batch_solid_step_each(hipStream_t, const BatchStep &, const BatchSolids &s, int, const BatchMember *, float *) { return note('E', 0, s); }
hipError_t launch_batch_solid_solve(hipStream_t, float *, const float *, const BatchSolids &s, int, int, int, int, SorParams) { return note('V', 0, s); }
hipError_t launch_batch_solid_solve_each(hipStream_t, float *, const float *, const BatchSolids &s, int, int, int, const BatchMember *, float *) { return note('W', 0, s); }
hipError_t launch_solid_velocity_stats(hipStream_t, FlowStatsRecord *, const float *, const BatchSolids &s, int, int, int, float, const float *) { return note('D', 0, s); }
hipError_t launch_flow_stats(hipStream_t, FlowStatsRecord *out, int what, const float *, const uint32_t *, int, int, int members, float, const float *)
{
    memset(out, 0, sizeof(FlowStatsRecord) * (size_t)members);
    return note('f', what);
}
hipError_t launch_update_norm(hipStream_t, unsigned *, const float *, const float *, Slab, int, int, float) { return hipSuccess; }
hipError_t launch_batch_render(hipStream_t, uint16_t *, const uint32_t *, int, int, int, int, bool) { return hipSuccess; }
hipError_t launch_history_sample(hipStream_t, const HistorySample &a, int)
{
    for (int k = 0; k < a.count; ++k) memset(&a.out[k], 0, sizeof a.out[k]);
    return note('H');
}
hipError_t launch_view_scalar(hipStream_t, float *out, const ViewFields &f, int what, float)
{
    memset(out, 0, (size_t)f.count * f.dim_x * f.dim_y * 4);
    return note('c', what);
}
hipError_t launch_view_texels(hipStream_t, uint32_t *out, const ViewFields &f, const ViewParams &v)
{
    memset(out, 0, (size_t)f.count * f.dim_x * f.dim_y * 12);
    return note('c', v.what);
}
hipError_t launch_view_render(hipStream_t, uint16_t *images, const ViewFields &f, const ViewParams &v, int scaling, bool)
{
    memset(images, 0, (size_t)f.count * scaling * (f.dim_x - 1) * scaling * (f.dim_y - 1) * 2);
    return note('c', v.what);
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
static bool info_is(sfl_batch *b, int set, int per_member)
{
    int s = -1, p = -1;
    return sfl_batch_solids_info(b, &s, &p) == SFL_OK && s == set && p == per_member;
}

static const int B = 3, X = 4, Y = 3, CELLS = X * Y;
// a hand-written mask of 4 x 3, row j = 0 first: a solid cell at (1, 0), one at (2, 1), one at (3, 2)
static const uint8_t MASK[CELLS] = {0, 1, 0, 0,
                                    0, 0, 7, 0,
                                    0, 0, 0, 1};
// ... and its code bytes, by hand: bit 0 W, 1 E, 2 S, 3 N present, bit 4 fluid
static const uint8_t CODES[CELLS] = {16 | 8,     0,          16 | 2,          16 | 1 | 8,
                                     16 | 2 | 4 | 8, 16 | 1 | 8, 0,           16 | 4,
                                     16 | 2 | 4, 16 | 1 | 2 | 4, 16 | 1,      0};

static void refusals_without_handles()
{
    uint8_t buf[CELLS];
    int w = 5;
    CHECK(sfl_batch_set_solids(nullptr, MASK, 2) == SFL_ERR_INVALID && says("per_member must be 0 or 1 (got 2)") && says("sfl_batch_set_solids"), "per_member 2: %s", sfl_last_error());
    CHECK(sfl_batch_set_solids(nullptr, MASK, 0) == SFL_ERR_INVALID && says("batch is NULL"), "NULL: %s", sfl_last_error());
    CHECK(sfl_batch_set_solids(nullptr, nullptr, 0) == SFL_ERR_INVALID && says("batch is NULL"), "NULL, clearing: %s", sfl_last_error());
    CHECK(sfl_batch_solids_info(nullptr, &w, &w) == SFL_ERR_INVALID && says("sfl_batch_solids_info: batch is NULL") && w == 5, "info: %s", sfl_last_error());
    CHECK(sfl_batch_solids_download(nullptr, 0, 1, buf, CELLS) == SFL_ERR_INVALID && says("sfl_batch_solids_download: batch is NULL"), "download: %s", sfl_last_error());
    CHECK(events.empty(), "a refused call launches nothing");
}

static void launchers_and_admission()
{
    sfl_batch *b = nullptr, *large = nullptr;
    CHECK(sfl_batch_create(&b, 0, X, Y, B) == SFL_OK && sfl_batch_create_large(&large, 0, X, Y, B) == SFL_OK && b && large, "create: %s", sfl_last_error());
    if (!b || !large) return;
    sfl_member_params prm[B];
    sfl_member_stop stop[B];
    for (int m = 0; m < B; ++m) {
        prm[m] = {DT * (m + 1), DX, OMEGA, 3 + m};
        stop[m] = {-1.0f, 2};
    }
    struct sfl_flow_stats stats[B];
    uint8_t got[B * CELLS];
    // ---- without solids: the old launchers
    events.clear();
    CHECK(info_is(b, 0, 0) && b->solids.step == nullptr && b->solids.solve == nullptr && b->solids.stats == nullptr, "no solids at first");
    CHECK(sfl_batch_step_n(b, 2, DT, DX, 4, OMEGA) == SFL_OK && sfl_batch_step_n_each(b, 1, prm) == SFL_OK && sfl_batch_poisson_solve(b, DX, 4, OMEGA) == SFL_OK &&
              sfl_batch_poisson_solve_each(b, prm) == SFL_OK && sfl_batch_flow_stats(b, 3, DX, 0, B, stats, sizeof stats) == SFL_OK && kinds() == "ssevwf" && events[5].n == 3,
          "without solids: %s (%s)", kinds().c_str(), sfl_last_error());
    CHECK(sfl_batch_solids_download(b, 0, B, got, sizeof got) == SFL_OK && std::string((char *)got, sizeof got) == std::string(sizeof got, '\0'), "no solids: zeros");
    // ---- the large batch: refused, with and without a mask
    CHECK(sfl_batch_set_solids(large, MASK, 0) == SFL_ERR_STATE && says("sfl_batch_create_large") && says("6144") && info_is(large, 0, 0) && large->solids.d_codes == nullptr,
          "large: %s", sfl_last_error());
    CHECK(sfl_batch_set_solids(large, MASK, 3) == SFL_ERR_INVALID && says("per_member"), "the argument check comes first: %s", sfl_last_error());
    // ---- a shared mask: the code bytes, the solid launchers, member stride 0
    events.clear();
    CHECK(sfl_batch_set_solids(b, MASK, 0) == SFL_OK && info_is(b, 1, 0) && events.empty() && b->solids.d_codes && b->solids.d_bytes == (size_t)CELLS,
          "set, shared: %s", sfl_last_error());
    CHECK(b->solids.d_codes && memcmp(b->solids.d_codes, CODES, CELLS) == 0, "the code bytes of the hand-written mask");
    CHECK(sfl_batch_step_n(b, 2, DT, DX, 4, OMEGA) == SFL_OK && sfl_batch_step_n_each(b, 1, prm) == SFL_OK && sfl_batch_poisson_solve(b, DX, 4, OMEGA) == SFL_OK &&
              sfl_batch_poisson_solve_each(b, prm) == SFL_OK && kinds() == "SSEVW", "with solids: %s (%s)", kinds().c_str(), sfl_last_error());
    for (const Event &e : events) CHECK(e.solids.codes == b->solids.d_codes && e.solids.member_stride == 0, "'%c' is handed the shared bytes", e.kind);
    float norm[B];
    CHECK(sfl_batch_residual(b, 0, B, norm, sizeof norm) == SFL_OK, "an _each call with solids leaves a report: %s", sfl_last_error());
    events.clear();
    CHECK(sfl_batch_flow_stats(b, 3, DX, 0, B, stats, sizeof stats) == SFL_OK && kinds() == "fD" && events[0].n == SFL_STATS_DYE, "statistics: %s", kinds().c_str());
    events.clear();
    CHECK(sfl_batch_flow_stats_each(b, SFL_STATS_VELOCITY, prm, 0, B, stats, sizeof stats) == SFL_OK && kinds() == "fD" && events[0].n == 0 && stats[0].what == SFL_STATS_VELOCITY,
          "velocity alone: the records zeroed, then the solids' pass: %s", kinds().c_str());
    events.clear();
    CHECK(sfl_batch_flow_stats(b, SFL_STATS_DYE, DX, 0, B, stats, sizeof stats) == SFL_OK && kinds() == "f" && events[0].n == SFL_STATS_DYE, "the dye alone is the old pass");
    CHECK(sfl_batch_solids_download(b, 1, 2, got, 2 * CELLS) == SFL_OK && got[1] == 1 && got[6] == 1 && got[11] == 1 && got[0] == 0 && memcmp(got, got + CELLS, CELLS) == 0,
          "download: 0 / 1 bytes, a shared mask repeated");
    CHECK(sfl_batch_solids_download(b, 1, 3, got, 3 * CELLS) == SFL_ERR_INVALID && says("not inside the batch's [0, 3)"), "range: %s", sfl_last_error());
    CHECK(sfl_batch_solids_download(b, 0, 2, got, CELLS) == SFL_ERR_INVALID && says("24 bytes, got 12"), "bytes: %s", sfl_last_error());
    CHECK(sfl_batch_solids_download(b, 0, 1, nullptr, CELLS) == SFL_ERR_INVALID && says("host is NULL"), "host: %s", sfl_last_error());
    // ---- a timeline that would be replayed in one launch runs a launch per step
    const int ms[2] = {0, 2}, cells[4] = {0, 0, 1, 0};   // (the second record names a solid cell: the kernel's business)
    const float vels[4] = {1, 0, 0, 1};
    const auto queue = [&] { return sfl_batch_queue_forces_at(b, 0, ms, cells, vels, 1) == SFL_OK && sfl_batch_queue_forces_at(b, 2, ms + 1, cells + 2, vels + 2, 1) == SFL_OK; };
    events.clear();
    CHECK(queue() && sfl_batch_step_n(b, 4, DT, DX, 4, OMEGA) == SFL_OK && kinds() == "SSSS", "a timeline with solids: %s", kinds().c_str());
    events.clear();
    CHECK(queue() && sfl_batch_step_n_each(b, 4, prm) == SFL_OK && kinds() == "EEEE", "... by the _each call: %s", kinds().c_str());
    // ---- per member: the stride is the member's cells; a smaller mask afterwards keeps the buffer
    uint8_t each[B * CELLS] = {};
    memcpy(each + CELLS, MASK, CELLS);   // member 0 and member 2: no solid cell
    events.clear();
    CHECK(sfl_batch_set_solids(b, each, 1) == SFL_OK && info_is(b, 1, 1) && b->solids.d_bytes == (size_t)B * CELLS && memcmp(b->solids.d_codes + CELLS, CODES, CELLS) == 0 &&
              b->solids.d_codes[0] == (16 | 2 | 8) && b->solids.d_codes[2 * CELLS + 5] == 31, "set, per member: %s", sfl_last_error());
    CHECK(sfl_batch_step_n(b, 1, DT, DX, 4, OMEGA) == SFL_OK && kinds() == "S" && events[0].solids.member_stride == (size_t)CELLS, "per member: the stride");
    CHECK(sfl_batch_solids_download(b, 0, B, got, sizeof got) == SFL_OK && got[CELLS + 6] == 1 && got[6] == 0 && got[2 * CELLS + 6] == 0, "download, per member");
    uint8_t *buffer = b->solids.d_codes;
    CHECK(sfl_batch_set_solids(b, MASK, 0) == SFL_OK && b->solids.d_codes == buffer && info_is(b, 1, 0), "a mask that needs no more keeps the buffer");
    // ---- admission: the call's own argument checks, then the state refusals, then (only then) anything staged
    CHECK(sfl_batch_poisson_solve_each(b, prm) == SFL_OK, "a report to keep");
    events.clear();
    sfl::BatchMember *members_before = b->d_members;
    const int slot_before = b->member_slot;
    CHECK(sfl_batch_step_n_until(b, -1, prm, stop) == SFL_ERR_INVALID && says("n must be >= 0"), "until: n first: %s", sfl_last_error());
    CHECK(sfl_batch_step_n_until(b, 2, prm, nullptr) == SFL_ERR_INVALID && says("stops is NULL"), "until: stops first: %s", sfl_last_error());
    CHECK(sfl_batch_step_n_until(b, 2, prm, stop) == SFL_ERR_STATE && says("sfl_batch_step_n_until") && says("solid cells set") && says("_each"), "until: %s", sfl_last_error());
    CHECK(sfl_batch_poisson_solve_until(b, nullptr, stop) == SFL_ERR_INVALID && says("params is NULL"), "solve_until: params first: %s", sfl_last_error());
    CHECK(sfl_batch_poisson_solve_until(b, prm, stop) == SFL_ERR_STATE && says("sfl_batch_poisson_solve_until") && says("solid cells set"), "solve_until: %s", sfl_last_error());
    CHECK(events.empty() && b->d_members == members_before && b->member_slot == slot_before, "a refused call stages and launches nothing");
    CHECK(sfl_batch_residual(b, 0, B, norm, sizeof norm) == SFL_OK, "... and leaves the report valid");
    // a history: its own checks first, then the refusal; a history that is on refuses a mask and lets a clear through
    CHECK(sfl_batch_history_start(b, 0, 0, B, 4) == SFL_ERR_INVALID && says("every must be >= 1"), "history: every first: %s", sfl_last_error());
    CHECK(sfl_batch_history_start(b, 1, 2, 2, 4) == SFL_ERR_INVALID && says("not inside the batch's"), "history: range first: %s", sfl_last_error());
    CHECK(sfl_batch_history_start(b, 1, 0, B, 4) == SFL_ERR_STATE && says("sfl_batch_history_start") && says("solid cells set") && !b->history.on && b->history_step == nullptr &&
              b->history.d_records == nullptr, "history: %s", sfl_last_error());
    CHECK(sfl_batch_set_solids(b, nullptr, 0) == SFL_OK && info_is(b, 0, 0) && b->solids.d_codes == nullptr && b->solids.step == nullptr, "clear");
    CHECK(sfl_batch_history_start(b, 1, 0, B, 4) == SFL_OK && b->history.on, "without solids a history starts: %s", sfl_last_error());
    CHECK(sfl_batch_set_solids(b, MASK, 5) == SFL_ERR_INVALID, "per_member first");
    CHECK(sfl_batch_set_solids(b, MASK, 0) == SFL_ERR_STATE && says("a history is on") && says("sfl_batch_history_stop") && info_is(b, 0, 0) && b->solids.d_codes == nullptr,
          "a mask while a history is on: %s", sfl_last_error());
    CHECK(sfl_batch_set_solids(b, nullptr, 0) == SFL_OK, "clearing is always let through");
    // ---- cleared: the old launchers again, the replay included
    events.clear();
    CHECK(sfl_batch_history_stop(b) == SFL_OK && queue() && sfl_batch_step_n(b, 4, DT, DX, 4, OMEGA) == SFL_OK && sfl_batch_step_n_each(b, 1, prm) == SFL_OK &&
              sfl_batch_poisson_solve(b, DX, 4, OMEGA) == SFL_OK && sfl_batch_poisson_solve_each(b, prm) == SFL_OK && sfl_batch_step_n_until(b, 1, prm, stop) == SFL_OK &&
              sfl_batch_poisson_solve_until(b, prm, stop) == SFL_OK && sfl_batch_flow_stats(b, 3, DX, 0, B, stats, sizeof stats) == SFL_OK && kinds() == "pevwuxf" &&
              events[0].n == 4 && events[6].n == 3, "cleared: %s (%s)", kinds().c_str(), sfl_last_error());
    // ---- the divergence view: the call's own checks first; the other views work; the recorder
    float scal[B * CELLS];
    static uint32_t colours[6] = {0, 0, 0, SFL_VIEW_MAX_COLOUR, 0, 0};
    sfl_view div{}, vort{};
    div.what = SFL_VIEW_DIVERGENCE, div.dx = DX, div.lo = -1, div.hi = 1, div.stops = 2, div.colours = colours;
    vort = div;
    vort.what = SFL_VIEW_VORTICITY;
    std::vector<uint32_t> tex((size_t)B * CELLS * 3);
    std::vector<uint16_t> img((size_t)B * (X - 1) * (Y - 1));
    CHECK(sfl_batch_set_solids(b, MASK, 0) == SFL_OK, "set again");
    events.clear();
    CHECK(sfl_batch_view_scalar(b, SFL_VIEW_DIVERGENCE, DX, 0, B, scal, 7) == SFL_ERR_INVALID && says("bytes"), "view: bytes first: %s", sfl_last_error());
    CHECK(sfl_batch_view_scalar(b, SFL_VIEW_DIVERGENCE, DX, 0, B, scal, sizeof scal) == SFL_ERR_STATE && says("sfl_batch_view_scalar") && says("divergence view") &&
              says("sfl_batch_flow_stats"), "view_scalar: %s", sfl_last_error());
    CHECK(sfl_batch_view_texels(b, &div, 0, B, tex.data(), tex.size() * 4) == SFL_ERR_STATE && says("sfl_batch_view_texels"), "view_texels: %s", sfl_last_error());
    CHECK(sfl_batch_view_render_members(b, &div, 0, B, 1, 0, img.data(), img.size() * 2) == SFL_ERR_STATE && says("sfl_batch_view_render_members"), "view_render: %s", sfl_last_error());
    CHECK(events.empty(), "a refused view launches nothing");
    CHECK(sfl_batch_view_scalar(b, SFL_VIEW_VORTICITY, DX, 0, B, scal, sizeof scal) == SFL_OK && sfl_batch_view_texels(b, &vort, 0, B, tex.data(), tex.size() * 4) == SFL_OK &&
              sfl_batch_view_scalar(b, SFL_VIEW_PRESSURE, DX, 0, B, scal, sizeof scal) == SFL_OK && kinds() == "ccc", "the other views: %s (%s)", kinds().c_str(), sfl_last_error());
    CHECK(sfl_batch_record_view(b, &div) == SFL_ERR_STATE && says("not recording"), "record_view: its own state first: %s", sfl_last_error());
    CHECK(sfl_batch_record_start(b, 1, 0, B, 1, 0, 8) == SFL_OK && sfl_batch_record_view(b, &div) == SFL_ERR_STATE && says("divergence view") && !b->rec.view_on,
          "record_view of the divergence: %s", sfl_last_error());
    CHECK(sfl_batch_record_view(b, &vort) == SFL_OK && b->rec.view_on && sfl_batch_step_n(b, 2, DT, DX, 4, OMEGA) == SFL_OK, "the vorticity is recorded: %s", sfl_last_error());
    // the recorder draws the divergence first, the mask comes second
    CHECK(sfl_batch_set_solids(b, nullptr, 0) == SFL_OK && sfl_batch_record_view(b, &div) == SFL_OK, "without solids the divergence is recorded");
    CHECK(sfl_batch_set_solids(b, MASK, 0) == SFL_ERR_STATE && says("recorder draws the divergence view") && info_is(b, 0, 0), "a mask while it is: %s", sfl_last_error());
    CHECK(sfl_batch_record_view(b, nullptr) == SFL_OK && sfl_batch_set_solids(b, MASK, 1 - 1) == SFL_OK && info_is(b, 1, 0), "the dye again: the mask is taken");
    // ---- destroy with solids set
    CHECK(sfl_batch_destroy(b) == SFL_OK && sfl_batch_destroy(large) == SFL_OK, "destroy");
    events.clear();
}

int main()
{
    refusals_without_handles();
    launchers_and_admission();
    const long left = fake_hip_live_allocations();
    printf("solids driver: %d failed checks, %ld allocations left\n", failures, left);
    return failures || left ? 1 : 0;
}
