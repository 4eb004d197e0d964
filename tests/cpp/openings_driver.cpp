// openings_driver.cpp -- TEST HARNESS (tests/cpp, `make -f openings.mk`; tests/test_openings.py): the HOST side of the openings
// (csrc/openings.cpp) and of its hooks in the step, solve and statistics calls (csrc/batch.cpp), in sfl_batch_set_solids
// (csrc/solids.cpp), the history's start (csrc/history.cpp), the views (csrc/views.cpp) and sfl_batch_set_viscosity
// (csrc/viscous.cpp), run on a box without a GPU: the host units of the batches over the runtime that lives on the host
// (fake_hip.cpp) and kernels that do nothing (launch_stubs_ok.cpp).  The launchers are stubs of THIS file that keep ONE log in
// the order of the calls.  What is checked: the open codes the device is handed for a hand-written map, without a mask, with
// one, and after the mask changes; the inflow staged and changed; which launcher each call picks and with which member stride;
// that the solids' code bytes stay what they were; that clearing restores the old launchers; the admission order -- a call's own
// argument checks, then the state refusals, each with its message, then (and only then) anything staged or launched; downloads
// and info; destroy with openings set leaves no allocation.  Exit status 0 and "0 failed checks".
//   openings_driver IN OUT     THE TILE CORE ON THE HOST: csrc/sor_solid_tile.h with csrc/sor_open_tile.h's set-up of k, one tile
//                              after the other against files of cases (run_tiles below; tests/test_openings.py)
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../esp32-fluid-simulation_amd/csrc/batch_state.h"
#include "../../esp32-fluid-simulation_amd/csrc/history_kernels.h"
#include "../../esp32-fluid-simulation_amd/csrc/sor_open_tile.h"
#include "../../esp32-fluid-simulation_amd/csrc/until_kernels.h"
#include "../../esp32-fluid-simulation_amd/csrc/view_kernels.h"
#include "../../esp32-fluid-simulation_amd/csrc/viscous_kernels.h"
#include "../../include/sfl.h"

extern "C" long fake_hip_live_allocations();
namespace sfl {
namespace host {
std::vector<uint8_t> solid_codes(const uint8_t *mask, int dim_x, int dim_y, size_t members);   // csrc/solids.cpp
int open_side(int i, int j, int dim_x, int dim_y);                                              // csrc/openings.cpp
}  // namespace host
}  // namespace sfl

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
    char kind;   // 's' 'e' 'u' a plain step (uniform, each, until), 'p' a replay, 'v' 'w' 'x' a plain solve; 'S' 'E' 'V' 'W' the same by
                 // the solids' rule, 'O' 'P' 'Q' 'R' by the openings'; 'f' the plain statistics, 'D' the solids' velocity pass, 'G' the
                 // openings'; 'B' a viscous step; 'H' a history's sample, 'c' a view's scalars
    int n;
    sfl::BatchOpenings open;
};
static std::vector<Event> events;
static hipError_t note(char kind, int n = 0, sfl::BatchOpenings o = {nullptr, 0, nullptr})
{
    events.push_back({kind, n, o});
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
hipError_t launch_batch_solid_step(hipStream_t, const BatchStep &, const BatchSolids &, int) { return note('S'); }
hipError_t launch_batch_solid_step_each(hipStream_t, const BatchStep &, const BatchSolids &, int, const BatchMember *, float *) { return note('E'); }
hipError_t launch_batch_solid_solve(hipStream_t, float *, const float *, const BatchSolids &, int, int, int, int, SorParams) { return note('V'); }
hipError_t launch_batch_solid_solve_each(hipStream_t, float *, const float *, const BatchSolids &, int, int, int, const BatchMember *, float *) { return note('W'); }
hipError_t launch_solid_velocity_stats(hipStream_t, FlowStatsRecord *, const float *, const BatchSolids &, int, int, int, float, const float *) { return note('D'); }
hipError_t launch_batch_open_step(hipStream_t, const BatchStep &, const BatchOpenings &o, int) { return note('O', 0, o); }
hipError_t launch_batch_open_step_each(hipStream_t, const BatchStep &, const BatchOpenings &o, int, const BatchMember *, float *) { return note('P', 0, o); }
hipError_t launch_batch_open_solve(hipStream_t, float *, const float *, const BatchOpenings &o, int, int, int, int, SorParams) { return note('Q', 0, o); }
hipError_t launch_batch_open_solve_each(hipStream_t, float *, const float *, const BatchOpenings &o, int, int, int, const BatchMember *, float *) { return note('R', 0, o); }
hipError_t launch_open_velocity_stats(hipStream_t, FlowStatsRecord *, const float *, const BatchOpenings &o, int, int, int, float, const float *) { return note('G', 0, o); }
hipError_t launch_batch_viscous_step(hipStream_t, const BatchStep &, const BatchViscous *, int) { return note('B'); }
hipError_t launch_batch_viscous_step_each(hipStream_t, const BatchStep &, const BatchViscous *, int, const BatchMember *, float *) { return note('B'); }
hipError_t launch_batch_viscous_solid_step(hipStream_t, const BatchStep &, const BatchSolids &, const BatchViscous *, int) { return note('B'); }
hipError_t launch_batch_viscous_solid_step_each(hipStream_t, const BatchStep &, const BatchSolids &, const BatchViscous *, int, const BatchMember *, float *) { return note('B'); }
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
static bool info_is(sfl_batch *b, int set, int per_member, int inflow_each, long long in, long long out)
{
    int s = -1, p = -1, q = -1;
    int64_t a = -1, c = -1;
    return sfl_batch_openings_info(b, &s, &p, &q, &a, &c) == SFL_OK && s == set && p == per_member && q == inflow_each && a == in && c == out;
}

static const int B = 3, X = 4, Y = 3, CELLS = X * Y;
static const int IN = SFL_OPEN_INFLOW, OUT = SFL_OPEN_OUTFLOW, OUTBIT = 1 << 12;
// a hand-written map of 4 x 3, row j = 0 first: an outflow to the south, an inflow in the west, an outflow in the east, an
// inflow to the north
static const uint8_t MAP[CELLS] = {0, OUT, 0, 0,
                                   IN, 0, 0, OUT,
                                   0, 0, IN, 0};
// ... its open codes on an all-fluid grid, by hand: the code byte (bit 0 W, 1 E, 2 S, 3 N present, 16 fluid), the open side << 8
static const uint16_t OPEN_CODES[CELLS] = {26, 27 | 4 << 8 | OUTBIT, 27, 25,
                                           30 | 1 << 8, 31, 31, 29 | 2 << 8 | OUTBIT,
                                           22, 23, 23 | 8 << 8, 21};
// the mask of solids_driver.cpp -- solid cells at (1, 0), (2, 1), (3, 2) -- and its code bytes
static const uint8_t MASK[CELLS] = {0, 1, 0, 0,
                                    0, 0, 7, 0,
                                    0, 0, 0, 1};
static const uint8_t CODES[CELLS] = {16 | 8,     0,          16 | 2,          16 | 1 | 8,
                                     16 | 2 | 4 | 8, 16 | 1 | 8, 0,           16 | 4,
                                     16 | 2 | 4, 16 | 1 | 2 | 4, 16 | 1,      0};
// ... and the open codes of MAP over MASK: the opening at the solid cell (1, 0) does not count
static const uint16_t MASKED_OPEN_CODES[CELLS] = {16 | 8, 0, 16 | 2, 16 | 1 | 8,
                                                  30 | 1 << 8, 16 | 1 | 8, 0, 20 | 2 << 8 | OUTBIT,
                                                  16 | 2 | 4, 16 | 1 | 2 | 4, 17 | 8 << 8, 0};
static const float INFLOW[2] = {3.5f, -0.0f};

static void refusals_without_handles()
{
    uint8_t buf[CELLS];
    float vel[2];
    const float nan[2] = {NAN, 0.0f};
    int w = 5;
    CHECK(sfl_batch_set_openings(nullptr, MAP, 2, INFLOW, 0) == SFL_ERR_INVALID && says("sfl_batch_set_openings: per_member must be 0 or 1 (got 2)"), "%s", sfl_last_error());
    CHECK(sfl_batch_set_openings(nullptr, MAP, 0, INFLOW, 7) == SFL_ERR_INVALID && says("inflow_per_member must be 0 or 1 (got 7)"), "%s", sfl_last_error());
    CHECK(sfl_batch_set_openings(nullptr, MAP, 0, nan, 0) == SFL_ERR_INVALID && says("must be finite"), "%s", sfl_last_error());
    CHECK(sfl_batch_set_openings(nullptr, MAP, 0, INFLOW, 0) == SFL_ERR_INVALID && says("batch is NULL"), "%s", sfl_last_error());
    CHECK(sfl_batch_set_inflow(nullptr, INFLOW, 0) == SFL_ERR_INVALID && says("sfl_batch_set_inflow: batch is NULL"), "%s", sfl_last_error());
    CHECK(sfl_batch_openings_info(nullptr, &w, &w, &w, nullptr, nullptr) == SFL_ERR_INVALID && says("sfl_batch_openings_info: batch is NULL") && w == 5, "%s", sfl_last_error());
    CHECK(sfl_batch_openings_download(nullptr, 0, 1, buf, CELLS) == SFL_ERR_INVALID && says("sfl_batch_openings_download: batch is NULL"), "%s", sfl_last_error());
    CHECK(sfl_batch_inflow_download(nullptr, 0, 1, vel, 8) == SFL_ERR_INVALID && says("sfl_batch_inflow_download: batch is NULL"), "%s", sfl_last_error());
    CHECK(events.empty(), "a refused call launches nothing");
}

static void maps_launchers_and_admission()
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
    float vel[2 * B];
    const std::string plain = "ssevwf";
    const auto all_calls = [&] {
        return sfl_batch_step_n(b, 2, DT, DX, 4, OMEGA) == SFL_OK && sfl_batch_step_n_each(b, 1, prm) == SFL_OK && sfl_batch_poisson_solve(b, DX, 4, OMEGA) == SFL_OK &&
               sfl_batch_poisson_solve_each(b, prm) == SFL_OK && sfl_batch_flow_stats(b, 3, DX, 0, B, stats, sizeof stats) == SFL_OK;
    };
    // ---- without openings: the old launchers, zeros from the downloads
    events.clear();
    CHECK(info_is(b, 0, 0, 0, 0, 0) && b->openings.step == nullptr && b->openings.restage == nullptr, "no openings at first");
    CHECK(all_calls() && kinds() == plain, "without openings: %s (%s)", kinds().c_str(), sfl_last_error());
    memset(got, 9, sizeof got);
    vel[0] = vel[5] = 9.0f;
    CHECK(sfl_batch_openings_download(b, 0, B, got, sizeof got) == SFL_OK && std::string((char *)got, sizeof got) == std::string(sizeof got, '\0'), "no openings: zeros");
    CHECK(sfl_batch_inflow_download(b, 0, B, vel, sizeof vel) == SFL_OK && vel[0] == 0.0f && vel[5] == 0.0f, "no openings: no inflow");
    CHECK(sfl_batch_set_inflow(b, INFLOW, 0) == SFL_ERR_STATE && says("no openings set"), "set_inflow without a map: %s", sfl_last_error());
    // ---- the map's own checks need the shape: each names the first bad cell
    uint8_t bad[CELLS];
    const auto with = [&](int cell, int value) {
        memset(bad, 0, sizeof bad);
        bad[cell] = (uint8_t)value;
        return bad;
    };
    events.clear();
    CHECK(sfl_batch_set_openings(b, with(0, IN), 0, INFLOW, 0) == SFL_ERR_INVALID && says("cell (0, 0)") && says("is a corner"), "corner: %s", sfl_last_error());
    CHECK(sfl_batch_set_openings(b, with(11, OUT), 0, INFLOW, 0) == SFL_ERR_INVALID && says("cell (3, 2)") && says("is a corner"), "corner: %s", sfl_last_error());
    CHECK(sfl_batch_set_openings(b, with(5, IN), 0, INFLOW, 0) == SFL_ERR_INVALID && says("cell (1, 1)") && says("interior cell"), "interior: %s", sfl_last_error());
    CHECK(sfl_batch_set_openings(b, with(4, 3), 0, INFLOW, 0) == SFL_ERR_INVALID && says("cell (0, 1) holds 3") && says("neither 0"), "a value of 3: %s", sfl_last_error());
    CHECK(sfl_batch_set_openings(b, MAP, 0, nullptr, 0) == SFL_ERR_INVALID && says("inflow is NULL"), "no inflow: %s", sfl_last_error());
    float each_nan[2 * B] = {1, 2, 3, INFINITY, 5, 6};
    CHECK(sfl_batch_set_openings(b, MAP, 0, each_nan, 1) == SFL_ERR_INVALID && says("member 1") && says("finite"), "a per-member inflow: %s", sfl_last_error());
    CHECK(info_is(b, 0, 0, 0, 0, 0) && b->openings.d_codes == nullptr && events.empty(), "nothing set by a refused call");
    // ---- the large batch: its argument checks first, then refused
    CHECK(sfl_batch_set_openings(large, with(0, IN), 0, INFLOW, 0) == SFL_ERR_INVALID, "large: the map's check comes first");
    CHECK(sfl_batch_set_openings(large, MAP, 0, INFLOW, 0) == SFL_ERR_STATE && says("sfl_batch_create_large") && says("6144") && large->openings.d_codes == nullptr, "large: %s", sfl_last_error());
    // ---- a shared map on an all-fluid grid: the open codes, the inflow, the openings' launchers, member stride 0
    events.clear();
    CHECK(sfl_batch_set_openings(b, MAP, 0, INFLOW, 0) == SFL_OK && info_is(b, 1, 0, 0, 2 * B, 2 * B) && events.empty(), "set, shared: %s", sfl_last_error());
    CHECK(b->openings.d_codes && memcmp(b->openings.d_codes, OPEN_CODES, sizeof OPEN_CODES) == 0, "the open codes of the hand-written map");
    CHECK(b->openings.d_inflow && memcmp(b->openings.d_inflow, INFLOW, 8) == 0 && memcmp(b->openings.d_inflow + 4, INFLOW, 8) == 0, "the inflow, repeated, -0.0f kept");
    int solids_set = 7;
    CHECK(sfl_batch_solids_info(b, &solids_set, nullptr) == SFL_OK && solids_set == 0 && b->solids.d_codes == nullptr, "solids_info still reports not set");
    CHECK(all_calls() && kinds() == "OOPQRfG" && events[5].n == SFL_STATS_DYE, "with openings: %s (%s)", kinds().c_str(), sfl_last_error());
    for (const Event &e : events)
        if (e.kind != 'f') CHECK(e.open.codes == b->openings.d_codes && e.open.member_stride == 0 && e.open.inflow == b->openings.d_inflow, "'%c' is handed the shared codes", e.kind);
    float norm[B];
    CHECK(sfl_batch_residual(b, 0, B, norm, sizeof norm) == SFL_OK, "an _each call with openings leaves a report: %s", sfl_last_error());
    CHECK(sfl_batch_openings_download(b, 1, 2, got, 2 * CELLS) == SFL_OK && memcmp(got, MAP, CELLS) == 0 && memcmp(got + CELLS, MAP, CELLS) == 0, "download: the map as given, repeated");
    CHECK(sfl_batch_openings_download(b, 1, 3, got, 3 * CELLS) == SFL_ERR_INVALID && says("not inside the batch's [0, 3)"), "range: %s", sfl_last_error());
    CHECK(sfl_batch_openings_download(b, 0, 2, got, CELLS) == SFL_ERR_INVALID && says("24 bytes, got 12"), "bytes: %s", sfl_last_error());
    CHECK(sfl_batch_openings_download(b, 0, 1, nullptr, CELLS) == SFL_ERR_INVALID && says("host is NULL"), "host: %s", sfl_last_error());
    CHECK(sfl_batch_inflow_download(b, 0, 2, vel, 8) == SFL_ERR_INVALID && says("16 bytes, got 8"), "inflow bytes: %s", sfl_last_error());
    CHECK(sfl_batch_inflow_download(b, 2, 2, vel, 16) == SFL_ERR_INVALID && says("not inside"), "inflow range: %s", sfl_last_error());
    CHECK(sfl_batch_inflow_download(b, 1, 2, vel, 16) == SFL_OK && memcmp(vel, INFLOW, 8) == 0 && memcmp(vel + 2, INFLOW, 8) == 0, "inflow download");
    // ---- the inflow changed without the map: per member
    const float sweep[2 * B] = {1, 0, 2, 0.5f, 3, -1};
    uint16_t *codes_before = b->openings.d_codes;
    events.clear();
    CHECK(sfl_batch_set_inflow(b, sweep, 1) == SFL_OK && info_is(b, 1, 0, 1, 2 * B, 2 * B) && b->openings.d_codes == codes_before && memcmp(b->openings.d_inflow, sweep, sizeof sweep) == 0 &&
              events.empty(), "set_inflow: %s", sfl_last_error());
    CHECK(sfl_batch_set_inflow(b, each_nan, 1) == SFL_ERR_INVALID && says("member 1") && memcmp(b->openings.d_inflow, sweep, sizeof sweep) == 0, "a refused inflow changes nothing");
    CHECK(sfl_batch_inflow_download(b, 0, B, vel, sizeof vel) == SFL_OK && memcmp(vel, sweep, sizeof sweep) == 0, "the sweep comes back");
    // ---- a timeline that would be replayed in one launch runs a launch per step
    const int ms[2] = {0, 2}, cells[4] = {0, 0, 1, 0};
    const float vels[4] = {1, 0, 0, 1};
    const auto queue = [&] { return sfl_batch_queue_forces_at(b, 0, ms, cells, vels, 1) == SFL_OK && sfl_batch_queue_forces_at(b, 2, ms + 1, cells + 2, vels + 2, 1) == SFL_OK; };
    events.clear();
    CHECK(queue() && sfl_batch_step_n(b, 4, DT, DX, 4, OMEGA) == SFL_OK && kinds() == "OOOO", "a timeline with openings: %s", kinds().c_str());
    // ---- a mask set afterwards: the open codes are formed again, the solids' bytes are the solids'
    CHECK(sfl_batch_set_solids(b, MASK, 0) == SFL_OK && info_is(b, 1, 0, 1, 2 * B, 1 * B), "a mask behind the map: %s", sfl_last_error());
    CHECK(memcmp(b->solids.d_codes, CODES, CELLS) == 0 && b->solids.d_bytes == (size_t)CELLS, "the code bytes of the solids are what they were");
    CHECK(memcmp(b->openings.d_codes, MASKED_OPEN_CODES, sizeof MASKED_OPEN_CODES) == 0, "the open codes over the mask");
    events.clear();
    CHECK(all_calls() && kinds() == "OOPQRfG", "with both: the openings' launchers: %s", kinds().c_str());
    // ... per member: the stride is the member's cells
    uint8_t each[B * CELLS] = {};
    memcpy(each + CELLS, MASK, CELLS);   // member 0 and member 2: no solid cell
    events.clear();
    CHECK(sfl_batch_set_solids(b, each, 1) == SFL_OK && info_is(b, 1, 0, 1, 2 * B, 2 * B - 1) && b->openings.d_bytes == sizeof(uint16_t) * B * CELLS, "a mask per member: %s", sfl_last_error());
    CHECK(memcmp(b->openings.d_codes, OPEN_CODES, sizeof OPEN_CODES) == 0 && memcmp(b->openings.d_codes + CELLS, MASKED_OPEN_CODES, sizeof OPEN_CODES) == 0 &&
              memcmp(b->openings.d_codes + 2 * CELLS, OPEN_CODES, sizeof OPEN_CODES) == 0, "the open codes of every member");
    CHECK(sfl_batch_step_n(b, 1, DT, DX, 4, OMEGA) == SFL_OK && kinds() == "O" && events[0].open.member_stride == (size_t)CELLS, "per member: the stride");
    // ... the mask cleared: all fluid again, shared again; the map set over a mask gives the same codes as the other order
    CHECK(sfl_batch_set_solids(b, nullptr, 0) == SFL_OK && info_is(b, 1, 0, 1, 2 * B, 2 * B) && memcmp(b->openings.d_codes, OPEN_CODES, sizeof OPEN_CODES) == 0, "the mask cleared");
    events.clear();
    CHECK(sfl_batch_step_n(b, 1, DT, DX, 4, OMEGA) == SFL_OK && kinds() == "O" && events[0].open.member_stride == 0, "shared again");
    CHECK(sfl_batch_set_openings(b, nullptr, 0, nullptr, 0) == SFL_OK && info_is(b, 0, 0, 0, 0, 0) && b->openings.d_codes == nullptr && b->openings.d_inflow == nullptr, "clear");
    CHECK(sfl_batch_set_solids(b, MASK, 0) == SFL_OK && sfl_batch_set_openings(b, MAP, 0, INFLOW, 0) == SFL_OK && info_is(b, 1, 0, 0, 2 * B, 1 * B) &&
              memcmp(b->openings.d_codes, MASKED_OPEN_CODES, sizeof MASKED_OPEN_CODES) == 0, "the map behind the mask: %s", sfl_last_error());
    // ... a map per member over a shared mask
    uint8_t maps[B * CELLS] = {};
    memcpy(maps + 2 * CELLS, MAP, CELLS);
    CHECK(sfl_batch_set_openings(b, maps, 1, INFLOW, 0) == SFL_OK && info_is(b, 1, 1, 0, 2, 1) && memcmp(b->openings.d_codes + 2 * CELLS, MASKED_OPEN_CODES, sizeof OPEN_CODES) == 0,
          "a map per member: %s", sfl_last_error());
    for (int c = 0; c < CELLS; ++c) CHECK(b->openings.d_codes[c] == CODES[c], "a member without an opening: the code bytes alone (cell %d)", c);
    CHECK(sfl_batch_openings_download(b, 0, B, got, sizeof got) == SFL_OK && memcmp(got, maps, sizeof maps) == 0, "download, per member");
    // ---- admission: the call's own argument checks, then the state refusals, then (only then) anything staged
    CHECK(sfl_batch_set_solids(b, nullptr, 0) == SFL_OK && sfl_batch_poisson_solve_each(b, prm) == SFL_OK, "a report to keep");
    events.clear();
    sfl::BatchMember *members_before = b->d_members;
    const int slot_before = b->member_slot;
    CHECK(sfl_batch_step_n_until(b, -1, prm, stop) == SFL_ERR_INVALID && says("n must be >= 0"), "until: n first: %s", sfl_last_error());
    CHECK(sfl_batch_step_n_until(b, 2, prm, stop) == SFL_ERR_STATE && says("sfl_batch_step_n_until") && says("openings set") && says("_each"), "until: %s", sfl_last_error());
    CHECK(sfl_batch_poisson_solve_until(b, nullptr, stop) == SFL_ERR_INVALID && says("params is NULL"), "solve_until: params first: %s", sfl_last_error());
    CHECK(sfl_batch_poisson_solve_until(b, prm, stop) == SFL_ERR_STATE && says("sfl_batch_poisson_solve_until") && says("openings set"), "solve_until: %s", sfl_last_error());
    CHECK(events.empty() && b->d_members == members_before && b->member_slot == slot_before, "a refused call stages and launches nothing");
    CHECK(sfl_batch_residual(b, 0, B, norm, sizeof norm) == SFL_OK, "... and leaves the report valid");
    // a history
    CHECK(sfl_batch_history_start(b, 0, 0, B, 4) == SFL_ERR_INVALID && says("every must be >= 1"), "history: every first: %s", sfl_last_error());
    CHECK(sfl_batch_history_start(b, 1, 0, B, 4) == SFL_ERR_STATE && says("sfl_batch_history_start") && says("openings set") && !b->history.on, "history: %s", sfl_last_error());
    // viscosity, in either order
    const float nu[1] = {0.1f};
    CHECK(sfl_batch_set_viscosity(b, nu, 0, -1) == SFL_ERR_INVALID && says("sweeps"), "viscosity: sweeps first: %s", sfl_last_error());
    CHECK(sfl_batch_set_viscosity(b, nu, 0, 2) == SFL_ERR_STATE && says("sfl_batch_set_viscosity") && says("openings set") && !b->viscosity.set, "viscosity behind openings: %s", sfl_last_error());
    CHECK(sfl_batch_set_openings(b, nullptr, 0, nullptr, 0) == SFL_OK && sfl_batch_set_viscosity(b, nu, 0, 2) == SFL_OK && b->viscosity.set, "viscosity without openings");
    CHECK(sfl_batch_set_openings(b, with(0, IN), 0, INFLOW, 0) == SFL_ERR_INVALID, "the map's check first");
    CHECK(sfl_batch_set_openings(b, MAP, 0, INFLOW, 0) == SFL_ERR_STATE && says("viscosity is set") && info_is(b, 0, 0, 0, 0, 0) && b->openings.d_codes == nullptr,
          "openings behind viscosity: %s", sfl_last_error());
    CHECK(sfl_batch_set_openings(b, nullptr, 0, nullptr, 0) == SFL_OK, "clearing is always let through");
    CHECK(sfl_batch_set_viscosity(b, nullptr, 0, 0) == SFL_OK, "viscosity cleared");
    // a history that is on refuses a map
    CHECK(sfl_batch_history_start(b, 1, 0, B, 4) == SFL_OK && b->history.on, "without openings a history starts: %s", sfl_last_error());
    CHECK(sfl_batch_set_openings(b, MAP, 0, INFLOW, 0) == SFL_ERR_STATE && says("a history is on") && says("sfl_batch_history_stop") && info_is(b, 0, 0, 0, 0, 0), "a map while a history is on: %s", sfl_last_error());
    // ---- cleared: the old launchers again, the replay included
    events.clear();
    CHECK(sfl_batch_history_stop(b) == SFL_OK && queue() && sfl_batch_step_n(b, 4, DT, DX, 4, OMEGA) == SFL_OK && sfl_batch_step_n_each(b, 1, prm) == SFL_OK &&
              sfl_batch_poisson_solve(b, DX, 4, OMEGA) == SFL_OK && sfl_batch_poisson_solve_each(b, prm) == SFL_OK && sfl_batch_step_n_until(b, 1, prm, stop) == SFL_OK &&
              sfl_batch_poisson_solve_until(b, prm, stop) == SFL_OK && sfl_batch_flow_stats(b, 3, DX, 0, B, stats, sizeof stats) == SFL_OK && kinds() == "pevwuxf" &&
              events[0].n == 4 && events[6].n == 3, "cleared: %s (%s)", kinds().c_str(), sfl_last_error());
    // ---- the divergence view and the recorder
    float scal[B * CELLS];
    static uint32_t colours[6] = {0, 0, 0, SFL_VIEW_MAX_COLOUR, 0, 0};
    sfl_view div{}, vort{};
    div.what = SFL_VIEW_DIVERGENCE, div.dx = DX, div.lo = -1, div.hi = 1, div.stops = 2, div.colours = colours;
    vort = div;
    vort.what = SFL_VIEW_VORTICITY;
    CHECK(sfl_batch_set_openings(b, MAP, 0, INFLOW, 0) == SFL_OK, "set again");
    events.clear();
    CHECK(sfl_batch_view_scalar(b, SFL_VIEW_DIVERGENCE, DX, 0, B, scal, 7) == SFL_ERR_INVALID && says("bytes"), "view: bytes first: %s", sfl_last_error());
    CHECK(sfl_batch_view_scalar(b, SFL_VIEW_DIVERGENCE, DX, 0, B, scal, sizeof scal) == SFL_ERR_STATE && says("sfl_batch_view_scalar") && says("openings set") && says("divergence view"),
          "view_scalar: %s", sfl_last_error());
    CHECK(events.empty(), "a refused view launches nothing");
    CHECK(sfl_batch_view_scalar(b, SFL_VIEW_VORTICITY, DX, 0, B, scal, sizeof scal) == SFL_OK && sfl_batch_view_scalar(b, SFL_VIEW_PRESSURE, DX, 0, B, scal, sizeof scal) == SFL_OK &&
              kinds() == "cc", "the other views: %s (%s)", kinds().c_str(), sfl_last_error());
    CHECK(sfl_batch_record_start(b, 1, 0, B, 1, 0, 8) == SFL_OK && sfl_batch_record_view(b, &div) == SFL_ERR_STATE && says("divergence view") && !b->rec.view_on,
          "record_view of the divergence: %s", sfl_last_error());
    CHECK(sfl_batch_record_view(b, &vort) == SFL_OK && b->rec.view_on && sfl_batch_step_n(b, 2, DT, DX, 4, OMEGA) == SFL_OK, "the vorticity is recorded: %s", sfl_last_error());
    CHECK(sfl_batch_set_openings(b, nullptr, 0, nullptr, 0) == SFL_OK && sfl_batch_record_view(b, &div) == SFL_OK, "without openings the divergence is recorded");
    CHECK(sfl_batch_set_openings(b, MAP, 0, INFLOW, 0) == SFL_ERR_STATE && says("recorder draws the divergence view") && info_is(b, 0, 0, 0, 0, 0), "a map while it is: %s", sfl_last_error());
    CHECK(sfl_batch_record_view(b, nullptr) == SFL_OK && sfl_batch_set_openings(b, MAP, 0, sweep, 1) == SFL_OK && info_is(b, 1, 0, 1, 2 * B, 2 * B), "the dye again: the map is taken");
    // ---- destroy with openings and solids set
    CHECK(sfl_batch_set_solids(b, MASK, 0) == SFL_OK, "solids for the end");
    CHECK(sfl_batch_destroy(b) == SFL_OK && sfl_batch_destroy(large) == SFL_OK, "destroy");
    events.clear();
}

// ---- the tile core on the host ---------------------------------------------------------------------------------------------
// openings_driver IN OUT: csrc/sor_solid_tile.h with csrc/sor_open_tile.h's set-up of k behind its load, run one workgroup's tile
// after the other, each phase thread after thread, with the launch segmentation of csrc/context_openings.cpp's solve.  IN: per
// case three int32 (dim_x, dim_y, iters), two floats (dx, omega), the right-hand side, the mask and the map; OUT: the pressures.
static int run_tiles(const char *in_path, const char *out_path)
{
    namespace st = sfl::solid_tile;
    FILE *in = fopen(in_path, "rb"), *out = fopen(out_path, "wb");
    if (!in || !out) return 2;
    std::vector<st::Cells> cells(st::kThreads);
    std::vector<float> lds(st::kLdsFloats);
    int cases = 0;
    for (;;) {
        int32_t head[3];
        float prm[2];
        if (fread(head, 4, 3, in) != 3) break;
        if (fread(prm, 4, 2, in) != 2) return 3;
        const int dim_x = head[0], dim_y = head[1], iters = head[2];
        const size_t n = (size_t)dim_x * dim_y;
        std::vector<float> d(n), p(n, 0.0f), alt(n, 0.0f);
        std::vector<uint8_t> mask(n), map(n), open(n, 0);
        if (fread(d.data(), 4, n, in) != n || fread(mask.data(), 1, n, in) != n || fread(map.data(), 1, n, in) != n) return 3;
        const std::vector<uint8_t> codes = sfl::host::solid_codes(mask.data(), dim_x, dim_y, 1);
        for (int j = 0; j < dim_y; ++j)   // the open byte, as csrc/context_openings.cpp forms it
            for (int i = 0; i < dim_x; ++i) {
                const size_t g = (size_t)j * dim_x + i;
                if (map[g] && (codes[g] & 16))
                    open[g] = (uint8_t)(sfl::host::open_side(i, j, dim_x, dim_y) | (map[g] == SFL_OPEN_OUTFLOW ? sfl::open_tile::kOpenOutflow : 0));
            }
        float *cur = p.data(), *next = alt.data();
        for (int l = 0; l < st::launches_of(iters); ++l) {
            st::Tile t;
            t.p_in = l == 0 ? nullptr : cur;
            t.p_out = next;
            t.d = d.data();
            t.codes = codes.data();
            t.dim_x = dim_x;
            t.dim_y = dim_y;
            t.k = st::iterations_of_launch(iters, l);
            t.dx = prm[0];
            t.omega = prm[1];
            t.one_minus_omega = 1.0f - prm[1];
            for (int ty = 0; ty < st::tiles_y(dim_y); ++ty)
                for (int tx = 0; tx < st::tiles_x(dim_x); ++tx) {
                    t.x0 = tx * st::kTX;
                    t.y0 = ty * st::kTY;
                    for (int tid = 0; tid < st::kThreads; ++tid) {
                        st::load(cells[tid], lds.data(), t, tid);
                        sfl::open_tile::set_up_k(cells[tid], t, open.data(), tid);
                    }
                    for (int it = 0; it < t.k; ++it)
                        for (int colour = 0; colour < 2; ++colour)
                            for (int tid = 0; tid < st::kThreads; ++tid) st::half_sweep(cells[tid], lds.data(), colour, t, tid);
                    for (int tid = 0; tid < st::kThreads; ++tid) st::store(cells[tid], t, tid);
                }
            std::swap(cur, next);
        }
        if (fwrite(cur, 4, n, out) != n) return 4;
        ++cases;
    }
    fclose(in);
    if (fclose(out) != 0) return 4;
    printf("openings driver: %d cases solved tile by tile (TX %d, TY %d, D %d)\n", cases, st::kTX, st::kTY, st::kD);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 3) return run_tiles(argv[1], argv[2]);
    refusals_without_handles();
    maps_launchers_and_admission();
    const long left = fake_hip_live_allocations();
    printf("openings driver: %d failed checks, %ld allocations left\n", failures, left);
    return failures || left ? 1 : 0;
}
