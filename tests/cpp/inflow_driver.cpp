// inflow_driver.cpp -- TEST HARNESS (tests/cpp, `make -f inflow.mk`; tests/test_inflow.py): the HOST side of the inflow
// profiles and of the flux (csrc/inflow.cpp and its two hooks in csrc/openings.cpp), run on a box without a GPU over the runtime
// that lives on the host (fake_hip.cpp) and kernels that do nothing (launch_stubs_ok.cpp).  The launchers are stubs of THIS file
// that keep one log.  What is checked: a record on a closed cell, an outflow cell, a corner or an interior cell is refused and
// named, with the member where a map per member lacks the cell; duplicates collapse to the later record; the table the device
// is handed (offsets, cells, velocities) for a shared and a per-member profile; a new map drops the profile and set_inflow
// keeps it; a mask change forms the table again; a refused call leaves the old profile; downloads in cell order; which step
// launcher a batch picks with and without a profile; the flux call's checks, its zeros without a launch and its record through
// the shared header; destroy leaves no allocation.  Exit status 0 and "0 failed checks".
//   inflow_driver IN OUT     THE FLUX ON THE HOST: csrc/open_flux.h's walk, term and reduction over files of cases (run_flux)
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../esp32-fluid-simulation_amd/csrc/batch_state.h"
#include "../../esp32-fluid-simulation_amd/csrc/history_kernels.h"
#include "../../esp32-fluid-simulation_amd/csrc/open_flux.h"
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

// ---- the log: 'O' 'P' the openings' step (uniform, each), 'I' 'J' the profile's, 'F' the flux, 's' 'e' a plain step ----------
struct Event {
    char kind;
    sfl::BatchProfile profile;
    int first, count;
};
static std::vector<Event> events;
static hipError_t note(char kind, sfl::BatchProfile p = {nullptr, nullptr, nullptr}, int first = 0, int count = 0)
{
    events.push_back({kind, p, first, count});
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
hipError_t launch_batch_play(hipStream_t, const BatchPlay &, int, const BatchMember *, float *) { return note('p'); }
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
hipError_t launch_batch_open_step(hipStream_t, const BatchStep &, const BatchOpenings &, int) { return note('O'); }
hipError_t launch_batch_open_step_each(hipStream_t, const BatchStep &, const BatchOpenings &, int, const BatchMember *, float *) { return note('P'); }
hipError_t launch_batch_open_solve(hipStream_t, float *, const float *, const BatchOpenings &, int, int, int, int, SorParams) { return note('Q'); }
hipError_t launch_batch_open_solve_each(hipStream_t, float *, const float *, const BatchOpenings &, int, int, int, const BatchMember *, float *) { return note('R'); }
hipError_t launch_open_velocity_stats(hipStream_t, FlowStatsRecord *, const float *, const BatchOpenings &, int, int, int, float, const float *) { return note('G'); }
hipError_t launch_batch_open_profile_step(hipStream_t, const BatchStep &, const BatchOpenings &, const BatchProfile &p, int) { return note('I', p); }
hipError_t launch_batch_open_profile_step_each(hipStream_t, const BatchStep &, const BatchOpenings &, const BatchProfile &p, int, const BatchMember *, float *)
{
    return note('J', p);
}
// the flux kernel's work, by the shared header, on the "device" memory that lives on the host
hipError_t launch_batch_open_flux(hipStream_t, struct sfl_open_flux *out, const float *v, const BatchOpenings &o, int dim_x, int dim_y, int first, int count)
{
    const size_t cells = (size_t)dim_x * dim_y;
    for (int k = 0; k < count; ++k) {
        const uint16_t *codes = o.codes + (size_t)(first + k) * o.member_stride;
        open_flux::flux_on_host(out + k, reinterpret_cast<const uint32_t *>(v) + 2 * (size_t)(first + k) * cells,
                                [codes](int c) { return (unsigned)codes[c] >> 8 & 31u; }, dim_x, dim_y);
    }
    return note('F', {nullptr, nullptr, nullptr}, first, count);
}
hipError_t launch_batch_viscous_step(hipStream_t, const BatchStep &, const BatchViscous *, int) { return note('B'); }
hipError_t launch_batch_viscous_step_each(hipStream_t, const BatchStep &, const BatchViscous *, int, const BatchMember *, float *) { return note('B'); }
hipError_t launch_batch_viscous_solid_step(hipStream_t, const BatchStep &, const BatchSolids &, const BatchViscous *, int) { return note('B'); }
hipError_t launch_batch_viscous_solid_step_each(hipStream_t, const BatchStep &, const BatchSolids &, const BatchViscous *, int, const BatchMember *, float *) { return note('B'); }
hipError_t launch_flow_stats(hipStream_t, FlowStatsRecord *out, int, const float *, const uint32_t *, int, int, int members, float, const float *)
{
    memset(out, 0, sizeof(FlowStatsRecord) * (size_t)members);
    return note('f');
}
hipError_t launch_update_norm(hipStream_t, unsigned *, const float *, const float *, Slab, int, int, float) { return hipSuccess; }
hipError_t launch_batch_render(hipStream_t, uint16_t *, const uint32_t *, int, int, int, int, bool) { return hipSuccess; }
hipError_t launch_history_sample(hipStream_t, const HistorySample &a, int)
{
    for (int k = 0; k < a.count; ++k) memset(&a.out[k], 0, sizeof a.out[k]);
    return note('H');
}
hipError_t launch_view_scalar(hipStream_t, float *, const ViewFields &, int, float) { return note('c'); }
hipError_t launch_view_texels(hipStream_t, uint32_t *, const ViewFields &, const ViewParams &) { return note('c'); }
hipError_t launch_view_render(hipStream_t, uint16_t *, const ViewFields &, const ViewParams &, int, bool) { return note('c'); }
}  // namespace sfl

static const float DT = 0.03f, DX = 0.7f, OMEGA = 1.9f;
static bool says(const char *word) { return strstr(sfl_last_error(), word) != nullptr; }
static std::string kinds()
{
    std::string s;
    for (const Event &e : events) s += e.kind;
    return s;
}

static const int B = 3, X = 5, Y = 4, CELLS = X * Y;
static const int IN = SFL_OPEN_INFLOW, OUT = SFL_OPEN_OUTFLOW;
// 5 x 4, row j = 0 first: inflow cells (0, 1), (0, 2) in the west and (2, 0) in the south, outflow cells (4, 1), (4, 2)
static const uint8_t MAP[CELLS] = {0, 0, IN, 0, 0,
                                   IN, 0, 0, 0, OUT,
                                   IN, 0, 0, 0, OUT,
                                   0, 0, 0, 0, 0};
static const float INFLOW[2] = {3.5f, 0.0f};

static bool profile_is(sfl_batch *b, int set, long long records)
{
    int s = -1;
    int64_t n = -1;
    return sfl_batch_inflow_profile_info(b, &s, &n) == SFL_OK && s == set && n == records;
}
// what member m's row of the device table holds
static std::string row_of(sfl_batch *b, int m)
{
    const sfl::BatchProfile &t = b->openings.profile_table;
    std::string s;
    char buf[64];
    for (int k = t.offsets[m]; k < t.offsets[m + 1]; ++k) {
        snprintf(buf, sizeof buf, "%u:(%g,%g) ", t.cells[k], (double)t.vel[2 * k], (double)t.vel[2 * k + 1]);
        s += buf;
    }
    return s;
}
static std::string held(sfl_batch *b, int m)
{
    int cells[2 * 16], n = -1;
    float vel[2 * 16];
    if (sfl_batch_inflow_profile_download(b, m, cells, vel, 16, &n) != SFL_OK) return "error";
    std::string s;
    char buf[64];
    for (int k = 0; k < n; ++k) {
        snprintf(buf, sizeof buf, "(%d,%d):(%g,%g) ", cells[2 * k], cells[2 * k + 1], (double)vel[2 * k], (double)vel[2 * k + 1]);
        s += buf;
    }
    return s;
}

static void refusals_without_handles()
{
    const int cells[4] = {0, 1, 0, 2};
    const float vel[4] = {1, 0, 2, 0}, nan[4] = {1, 0, NAN, 0}, inf[4] = {INFINITY, 0, 2, 0};
    struct sfl_open_flux rec;
    int n = 5;
    int64_t w = 5;
    CHECK(sfl_batch_set_inflow_profile(nullptr, nullptr, cells, vel, -1) == SFL_ERR_INVALID && says("sfl_batch_set_inflow_profile: n must be >= 0 (got -1)"), "%s", sfl_last_error());
    CHECK(sfl_batch_set_inflow_profile(nullptr, nullptr, nullptr, vel, 2) == SFL_ERR_INVALID && says("cells_ij is NULL with n = 2"), "%s", sfl_last_error());
    CHECK(sfl_batch_set_inflow_profile(nullptr, nullptr, cells, nullptr, 2) == SFL_ERR_INVALID && says("vel_xy is NULL with n = 2"), "%s", sfl_last_error());
    CHECK(sfl_batch_set_inflow_profile(nullptr, nullptr, cells, nan, 2) == SFL_ERR_INVALID && says("must be finite (record 1: (nan, 0))"), "%s", sfl_last_error());
    CHECK(sfl_batch_set_inflow_profile(nullptr, nullptr, cells, inf, 2) == SFL_ERR_INVALID && says("must be finite (record 0: (inf, 0))"), "%s", sfl_last_error());
    CHECK(sfl_batch_set_inflow_profile(nullptr, nullptr, cells, vel, 2) == SFL_ERR_INVALID && says("sfl_batch_set_inflow_profile: batch is NULL"), "%s", sfl_last_error());
    CHECK(sfl_batch_inflow_profile_info(nullptr, &n, &w) == SFL_ERR_INVALID && says("sfl_batch_inflow_profile_info: batch is NULL") && n == 5 && w == 5, "%s", sfl_last_error());
    CHECK(sfl_batch_inflow_profile_download(nullptr, 0, nullptr, nullptr, 0, &n) == SFL_ERR_INVALID && says("sfl_batch_inflow_profile_download: batch is NULL"), "%s", sfl_last_error());
    CHECK(sfl_batch_openings_flux(nullptr, 0, 1, &rec, sizeof rec) == SFL_ERR_INVALID && says("sfl_batch_openings_flux: batch is NULL"), "%s", sfl_last_error());
    CHECK(events.empty(), "a refused call launches nothing");
}

static void profiles()
{
    sfl_batch *b = nullptr, *large = nullptr;
    CHECK(sfl_batch_create(&b, 0, X, Y, B) == SFL_OK && sfl_batch_create_large(&large, 0, X, Y, B) == SFL_OK && b && large, "create: %s", sfl_last_error());
    if (!b || !large) return;
    sfl_member_params prm[B];
    for (int m = 0; m < B; ++m) prm[m] = {DT * (m + 1), DX, OMEGA, 3 + m};
    const auto steps = [&] { return sfl_batch_step_n(b, 2, DT, DX, 4, OMEGA) == SFL_OK && sfl_batch_step_n_each(b, 1, prm) == SFL_OK; };
    const int cells[6] = {0, 1, 0, 2, 2, 0};   // (0, 1) = cell 5, (0, 2) = cell 10, (2, 0) = cell 2
    const float vel[6] = {1, 0.5f, 2, -0.0f, 0.25f, 4};
    struct sfl_open_flux flux[B];
    // ---- admission: without openings, on a large batch
    events.clear();
    CHECK(profile_is(b, 0, 0) && held(b, 0).empty(), "no profile at first");
    CHECK(sfl_batch_set_inflow_profile(b, nullptr, nullptr, nullptr, 0) == SFL_OK && profile_is(b, 0, 0), "clearing nothing is let through");
    CHECK(sfl_batch_set_inflow_profile(b, nullptr, cells, vel, 3) == SFL_ERR_STATE && says("no openings set") && says("sfl_batch_set_openings"), "%s", sfl_last_error());
    const int outside[1] = {3};
    CHECK(sfl_batch_set_inflow_profile(large, outside, cells, vel, 1) == SFL_ERR_INVALID && says("record 0 names member 3") && says("[0, 3)"), "the member first: %s", sfl_last_error());
    CHECK(sfl_batch_set_inflow_profile(large, nullptr, cells, vel, 1) == SFL_ERR_STATE && says("sfl_batch_create_large"), "%s", sfl_last_error());
    memset(flux, 9, sizeof flux);
    CHECK(sfl_batch_openings_flux(b, 0, B, flux, sizeof flux) == SFL_OK && std::string((char *)flux, sizeof flux) == std::string(sizeof flux, '\0') && events.empty(),
          "no openings: zero records without a launch");
    CHECK(sfl_batch_openings_flux(b, 0, B, flux, 40) == SFL_ERR_INVALID && says("120 bytes, got 40"), "%s", sfl_last_error());
    CHECK(sfl_batch_openings_flux(b, 2, 2, flux, 80) == SFL_ERR_INVALID && says("not inside the batch's [0, 3)"), "%s", sfl_last_error());
    CHECK(sfl_batch_openings_flux(b, 0, 1, nullptr, 40) == SFL_ERR_INVALID && says("host is NULL"), "%s", sfl_last_error());
    // ---- a shared map: the records against it, each refusal naming the record
    CHECK(sfl_batch_set_openings(b, MAP, 0, INFLOW, 0) == SFL_OK, "the map: %s", sfl_last_error());
    const auto one = [&](int i, int j) {
        const int c[4] = {0, 1, i, j};
        const float v[4] = {1, 1, 2, 2};
        return sfl_batch_set_inflow_profile(b, nullptr, c, v, 2);
    };
    CHECK(one(1, 1) == SFL_ERR_INVALID && says("record 1 names cell (1, 1)") && says("map byte is 0"), "an interior cell: %s", sfl_last_error());
    CHECK(one(3, 0) == SFL_ERR_INVALID && says("record 1 names cell (3, 0)") && says("map byte is 0"), "a closed rim cell: %s", sfl_last_error());
    CHECK(one(4, 1) == SFL_ERR_INVALID && says("record 1 names cell (4, 1)") && says("map byte is 2, not SFL_OPEN_INFLOW"), "an outflow cell: %s", sfl_last_error());
    CHECK(one(0, 0) == SFL_ERR_INVALID && says("record 1 names cell (0, 0)"), "a corner: %s", sfl_last_error());
    CHECK(one(5, 1) == SFL_ERR_INVALID && says("record 1 names cell (5, 1)") && says("not inside the grid of 5 x 4"), "outside: %s", sfl_last_error());
    CHECK(profile_is(b, 0, 0) && b->openings.d_profile == nullptr && b->openings.profile_step == nullptr, "nothing set by a refused call");
    events.clear();
    CHECK(steps() && kinds() == "OOP", "openings without a profile: the openings' own launchers (%s)", kinds().c_str());
    // ---- a shared profile with a duplicate: the later record wins, rows in cell order, every member the same row
    const int dup_cells[8] = {0, 2, 0, 1, 2, 0, 0, 2};
    const float dup_vel[8] = {9, 9, 1, 0.5f, 0.25f, 4, 2, -0.0f};
    CHECK(sfl_batch_set_inflow_profile(b, nullptr, dup_cells, dup_vel, 4) == SFL_OK && profile_is(b, 1, 3 * B), "a shared profile: %s", sfl_last_error());
    CHECK(held(b, 1) == "(2,0):(0.25,4) (0,1):(1,0.5) (0,2):(2,-0) ", "downloads in cell order, the later record kept: %s", held(b, 1).c_str());
    for (int m = 0; m < B; ++m) CHECK(row_of(b, m) == "2:(0.25,4) 5:(1,0.5) 10:(2,-0) ", "member %d's row: %s", m, row_of(b, m).c_str());
    int n = -1, two[4];
    float two_v[4];
    CHECK(sfl_batch_inflow_profile_download(b, 0, two, two_v, 2, &n) == SFL_ERR_INVALID && n == 3 && says("holds 3 records, the arrays have room for 2"), "%s", sfl_last_error());
    events.clear();
    CHECK(steps() && kinds() == "IIJ" && events[0].profile.offsets == b->openings.profile_table.offsets, "with a profile: its launchers (%s)", kinds().c_str());
    // ---- set_inflow keeps it; a refused call leaves it
    const void *table = b->openings.d_profile;
    CHECK(sfl_batch_set_inflow(b, INFLOW, 0) == SFL_OK && profile_is(b, 1, 3 * B) && b->openings.d_profile == table, "set_inflow keeps the profile");
    CHECK(one(4, 2) == SFL_ERR_INVALID && profile_is(b, 1, 3 * B) && held(b, 2) == "(2,0):(0.25,4) (0,1):(1,0.5) (0,2):(2,-0) " &&
              row_of(b, 2) == "2:(0.25,4) 5:(1,0.5) 10:(2,-0) ", "a refused call leaves the old profile in place");
    // ---- a mask change forms the table again: the record on the solid inflow cell (0, 1) has no effect but is kept
    uint8_t mask[CELLS] = {};
    mask[5] = 1;
    CHECK(sfl_batch_set_solids(b, mask, 0) == SFL_OK && profile_is(b, 1, 3 * B), "a mask behind the profile: %s", sfl_last_error());
    for (int m = 0; m < B; ++m) CHECK(row_of(b, m) == "2:(0.25,4) 10:(2,-0) ", "member %d's row over the mask: %s", m, row_of(b, m).c_str());
    uint8_t each[B * CELLS] = {};
    each[CELLS + 10] = 1;   // member 1 alone: (0, 2) solid
    CHECK(sfl_batch_set_solids(b, each, 1) == SFL_OK, "a mask per member: %s", sfl_last_error());
    CHECK(row_of(b, 0) == "2:(0.25,4) 5:(1,0.5) 10:(2,-0) " && row_of(b, 1) == "2:(0.25,4) 5:(1,0.5) " && row_of(b, 2) == row_of(b, 0), "rows by the members' masks: %s | %s", row_of(b, 0).c_str(),
          row_of(b, 1).c_str());
    events.clear();
    CHECK(steps() && kinds() == "IIJ", "still the profile's launchers (%s)", kinds().c_str());
    CHECK(sfl_batch_set_solids(b, nullptr, 0) == SFL_OK && row_of(b, 1) == "2:(0.25,4) 5:(1,0.5) 10:(2,-0) ", "the mask cleared: the record counts again");
    // ---- records per member
    const int who[3] = {2, 0, 2};
    CHECK(sfl_batch_set_inflow_profile(b, who, cells, vel, 3) == SFL_OK && profile_is(b, 1, 3), "per member: %s", sfl_last_error());
    CHECK(row_of(b, 0) == "10:(2,-0) " && row_of(b, 1).empty() && row_of(b, 2) == "2:(0.25,4) 5:(1,0.5) ", "rows per member: %s | %s | %s", row_of(b, 0).c_str(), row_of(b, 1).c_str(),
          row_of(b, 2).c_str());
    CHECK(held(b, 1).empty() && held(b, 2) == "(2,0):(0.25,4) (0,1):(1,0.5) ", "downloads per member");
    // ---- clearing: the openings' own launchers again
    events.clear();
    CHECK(sfl_batch_set_inflow_profile(b, nullptr, nullptr, nullptr, 0) == SFL_OK && profile_is(b, 0, 0) && b->openings.d_profile == nullptr && steps() && kinds() == "OOP", "cleared: %s",
          kinds().c_str());
    // ---- a new map drops the profile
    CHECK(sfl_batch_set_inflow_profile(b, nullptr, cells, vel, 3) == SFL_OK && profile_is(b, 1, 3 * B), "set again");
    CHECK(sfl_batch_set_openings(b, MAP, 0, INFLOW, 0) == SFL_OK && profile_is(b, 0, 0) && b->openings.d_profile == nullptr && b->openings.profile_step == nullptr, "a new map drops the profile");
    // ---- a map per member where one member lacks the cell: refused, naming the member
    uint8_t maps[B * CELLS];
    for (int m = 0; m < B; ++m) memcpy(maps + m * CELLS, MAP, CELLS);
    maps[1 * CELLS + 10] = 0;   // member 1: (0, 2) closed
    CHECK(sfl_batch_set_openings(b, maps, 1, INFLOW, 0) == SFL_OK, "maps per member: %s", sfl_last_error());
    CHECK(sfl_batch_set_inflow_profile(b, nullptr, cells, vel, 3) == SFL_ERR_INVALID && says("record 1 names cell (0, 2)") && says("in member 1 is 0"), "the member is named: %s", sfl_last_error());
    const int not_one[3] = {0, 2, 1};
    CHECK(sfl_batch_set_inflow_profile(b, not_one, cells, vel, 3) == SFL_OK && profile_is(b, 1, 3), "records that avoid member 1's closed cell: %s", sfl_last_error());
    const int on_one[1] = {1};
    CHECK(sfl_batch_set_inflow_profile(b, on_one, cells + 2, vel + 2, 1) == SFL_ERR_INVALID && says("record 0") && says("in member 1 is 0") && profile_is(b, 1, 3), "%s", sfl_last_error());
    // ---- the flux through the launcher above: a known field
    CHECK(sfl_batch_set_openings(b, MAP, 0, INFLOW, 0) == SFL_OK, "shared again");
    std::vector<float> v(2 * (size_t)B * CELLS, 0.0f);
    for (int m = 0; m < B; ++m) {
        float *q = v.data() + 2 * (size_t)m * CELLS;
        q[2 * 5] = 1.0f * (m + 1);      // (0, 1): enters with 1, 2, 3
        q[2 * 10] = 0.5f;               // (0, 2): enters with 0.5
        q[2 * 2 + 1] = 0.25f;           // (2, 0): enters with 0.25 through the south
        q[2 * 9] = 1.5f;                // (4, 1): leaves with 1.5
        q[2 * 14] = -0.25f;             // (4, 2): comes back in with 0.25
    }
    CHECK(sfl_batch_upload(b, SFL_FIELD_VELOCITY, 0, B, v.data(), v.size() * sizeof(float)) == SFL_OK, "upload: %s", sfl_last_error());
    events.clear();
    CHECK(sfl_batch_openings_flux(b, 1, 2, flux, 80) == SFL_OK && kinds() == "F" && events[0].first == 1 && events[0].count == 2, "the flux of members 1 and 2: %s", sfl_last_error());
    // member 1: the maximum is 2.0 = 2^1, q = -31; 2.75 enters, 1.25 leaves
    CHECK(flux[0].exp2 == -31 && flux[0].max_abs_n == 2.0f && flux[0].inflow == (int64_t)(2.75 * 2147483648.0) && flux[0].outflow == (int64_t)(1.25 * 2147483648.0) &&
              flux[0].inflow_cells == 3 && flux[0].outflow_cells == 2 && flux[0].nonfinite == 0 && flux[0].reserved == 0,
          "member 1: %lld %lld %d", (long long)flux[0].inflow, (long long)flux[0].outflow, flux[0].exp2);
    CHECK(flux[1].exp2 == -31 && flux[1].max_abs_n == 3.0f && flux[1].inflow == (int64_t)(3.75 * 2147483648.0), "member 2: %lld %d", (long long)flux[1].inflow, flux[1].exp2);
    // every open cell solid: zeros without a launch
    uint8_t rim[CELLS] = {};
    for (int c = 0; c < CELLS; ++c) rim[c] = MAP[c] ? 1 : 0;
    events.clear();
    memset(flux, 9, sizeof flux);
    CHECK(sfl_batch_set_solids(b, rim, 0) == SFL_OK && sfl_batch_openings_flux(b, 0, B, flux, sizeof flux) == SFL_OK && events.empty() &&
              std::string((char *)flux, sizeof flux) == std::string(sizeof flux, '\0'), "no live open cell: zeros without a launch");
    // ---- destroy with a profile and a flux buffer held
    CHECK(sfl_batch_set_solids(b, nullptr, 0) == SFL_OK && sfl_batch_set_inflow_profile(b, nullptr, cells, vel, 3) == SFL_OK && b->openings.d_flux != nullptr, "a profile for the end");
    CHECK(sfl_batch_destroy(b) == SFL_OK && sfl_batch_destroy(large) == SFL_OK, "destroy");
    events.clear();
}

// ---- the flux on the host ---------------------------------------------------------------------------------------------------
// inflow_driver IN OUT: per case two int32 (dim_x, dim_y), the velocity (2 floats per cell), the mask and the map (a byte per
// cell each); OUT: one 40-byte record per case, by csrc/open_flux.h over the open bits formed as the host units form them.
static int run_flux(const char *in_path, const char *out_path)
{
    FILE *in = fopen(in_path, "rb"), *out = fopen(out_path, "wb");
    if (!in || !out) return 2;
    int cases = 0;
    for (;;) {
        int32_t head[2];
        if (fread(head, 4, 2, in) != 2) break;
        const int dim_x = head[0], dim_y = head[1];
        const size_t n = (size_t)dim_x * dim_y;
        std::vector<uint32_t> v(2 * n);
        std::vector<uint8_t> mask(n), map(n), open(n, 0);
        if (fread(v.data(), 4, 2 * n, in) != 2 * n || fread(mask.data(), 1, n, in) != n || fread(map.data(), 1, n, in) != n) return 3;
        const std::vector<uint8_t> codes = sfl::host::solid_codes(mask.data(), dim_x, dim_y, 1);
        for (int j = 0; j < dim_y; ++j)
            for (int i = 0; i < dim_x; ++i) {
                const size_t g = (size_t)j * dim_x + i;
                if (map[g] && (codes[g] & 16)) open[g] = (uint8_t)(sfl::host::open_side(i, j, dim_x, dim_y) | (map[g] == SFL_OPEN_OUTFLOW ? 16 : 0));
            }
        struct sfl_open_flux rec;
        const uint8_t *bits = open.data();
        sfl::open_flux::flux_on_host(&rec, v.data(), [bits](int c) { return (unsigned)bits[c]; }, dim_x, dim_y);
        if (fwrite(&rec, sizeof rec, 1, out) != 1) return 4;
        ++cases;
    }
    fclose(in);
    if (fclose(out) != 0) return 4;
    printf("inflow driver: %d flux records by the shared header\n", cases);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 3) return run_flux(argv[1], argv[2]);
    refusals_without_handles();
    profiles();
    const long left = fake_hip_live_allocations();
    printf("inflow driver: %d failed checks, %ld allocations left\n", failures, left);
    return failures || left ? 1 : 0;
}
