// walls_driver.cpp -- TEST HARNESS (tests/cpp, `make -f walls.mk`; tests/test_walls.py): the HOST side of the wall velocities
// (csrc/walls.cpp, csrc/context_walls.cpp, csrc/wall_table.h) and of their hooks in the step calls and in sfl_[batch_]set_solids,
// run on a box without a GPU: the host units over the runtime that lives on the host (fake_hip.cpp) and kernels that do nothing
// (launch_stubs_ok.cpp).  The launchers the calls end in are stubs of THIS file that keep ONE log in the order of the calls,
// which is the order of the stream.  What is checked:
//   * wall_table.h on its own: the first offending record and its member, later-wins deduplication, cell order, the CSR rows of
//     a shared and a per-member table, a member without records;
//   * a batch: the table the device is handed (offsets, cells, velocities) for a shared table, a per-member table and per-member
//     masks; which step launcher runs with and without a table and with and without a viscosity; a refused call leaves the table
//     and launches nothing; n == 0 clears; every sfl_batch_set_solids, a clear included, drops the table; downloads in cell order;
//   * a context: the compact list; the order of the launches of a step with a table, without a viscosity (the solids' step, then
//     the scatter) and with one (the launch over the code bytes in front of the diffusion, which then does not zero the solids;
//     the scatter last); step_n is n such steps; refusals; a new mask drops the table;
//   * with openings (csrc/openings.cpp, csrc/inflow.cpp, csrc/context_openings.cpp): a batch logs the walls' step on open codes
//     with the wall table and no profile's table, then with the profile's; a context logs the openings' step and the scatter
//     behind it; setting and clearing openings around a held table keeps the table and re-hooks the step; a refusal and a clear
//     under openings leave the table as it was;
//   * destroy leaves no allocation.
// Exit status 0 and "0 failed checks".
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../esp32-fluid-simulation_amd/csrc/batch_state.h"
#include "../../esp32-fluid-simulation_amd/csrc/diffuse_tile.h"
#include "../../esp32-fluid-simulation_amd/csrc/history_kernels.h"
#include "../../esp32-fluid-simulation_amd/csrc/open_kernels.h"
#include "../../esp32-fluid-simulation_amd/csrc/solid_kernels.h"
#include "../../esp32-fluid-simulation_amd/csrc/stats_kernels.h"
#include "../../esp32-fluid-simulation_amd/csrc/until_kernels.h"
#include "../../esp32-fluid-simulation_amd/csrc/view_kernels.h"
#include "../../esp32-fluid-simulation_amd/csrc/viscous_kernels.h"
#include "../../esp32-fluid-simulation_amd/csrc/wall_kernels.h"
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
// A context's: 'a' velocity advection, 'c' dye advection, 'f' forces, 'D' 'S' 'G' divergence, solve launch and gradient by the
// solids' rule (n of 'D': zero_solids), 'V' a launch of the diffusion (n: zero_solids), 'I' the launch over the code bytes, 'W'
// the scatter (n: the records), 'i' the openings' item 2a (n: with a profile), 'd' 's' 'g' divergence, solve launch and gradient by
// the openings' rule (n of 'd': zero_solids), anything else 'x'.  A batch's: 'b' a solids step, 'B' a viscous one, 'o' an openings'
// step (n: each | profile << 1), 'L' a walls step on the solids' bytes (n: each | viscous << 1; table: what it was handed), 'O' a
// walls step on open codes (n: each; table: the walls', profile: the profile's as handed).
struct Event {
    char kind;
    int n;
    const void *v;
    sfl::BatchProfile table, profile;
};
static std::vector<Event> events;
static hipError_t note(char kind, int n = 0, const void *v = nullptr, sfl::BatchProfile table = {nullptr, nullptr, nullptr},
                       sfl::BatchProfile profile = {nullptr, nullptr, nullptr})
{
    events.push_back({kind, n, v, table, profile});
    return hipSuccess;
}

namespace sfl {
bool small_grid_fits(int dim_x, int dim_y)   // (the real rule of small_grid.hip; launch_stubs_ok.cpp's answer is "no")
{
    return dim_x >= 2 && dim_y >= 2 && (long long)dim_x * dim_y <= kSmallGridMaxCells &&
           (long long)dim_y * ((dim_x + 1) / 2) <= kSmallGridMaxCells / 2;
}
// ---- what a context's calls end in
hipError_t launch_advect_vec2f(hipStream_t, float *, const float *, const float *, Slab, int, int, int, int, float, bool, int *, const Slab *, int, int, int) { return note('a'); }
hipError_t launch_advect_vec3uq32(hipStream_t, uint32_t *, const uint32_t *, const float *, Slab, int, int, int, int, float, bool, int *, const Slab *, int) { return note('c'); }
hipError_t launch_advect_divergence_tiled(hipStream_t, float *, float *, const float *, Slab, float, bool, float) { return note('x'); }
hipError_t launch_project_advect_vec3uq32(hipStream_t, uint32_t *, const uint32_t *, float *, const float *, Slab, int, int, int, int, float, bool, int *, float, int, bool *) { return note('x'); }
hipError_t launch_step_seam_tiled(hipStream_t, uint32_t *, const uint32_t *, float *, float *, const float *, const float *, Slab, float, float) { return note('x'); }
hipError_t launch_apply_forces(hipStream_t, float *, Slab, int, int, const int *, const float *, int n) { return note('f', n); }
hipError_t launch_divergence(hipStream_t, float *, const float *, Slab, int, int, float, int) { return note('x'); }
hipError_t launch_subtract_gradient(hipStream_t, float *, const float *, Slab, int, int, float, int) { return note('x'); }
hipError_t launch_sor_half_sweep(hipStream_t, float *, const float *, Slab, int, int, int, SorParams) { return note('x'); }
hipError_t launch_sor_fused(hipStream_t, float *, const float *, const float *, Slab, SorRows, int, int, SorParams, int, int, const HaloWait *, int *senders)
{
    if (senders) *senders = 0;
    return note('x');
}
hipError_t launch_zero_rows(hipStream_t, float *, Slab, int, int) { return note('x'); }
hipError_t launch_small_step(hipStream_t, const SmallStep &) { return note('x'); }
hipError_t launch_small_solve(hipStream_t, float *, const float *, int, int, int, SorParams) { return note('x'); }
hipError_t launch_small_solve_warm(hipStream_t, float *, const float *, int, int, int, SorParams) { return note('x'); }
hipError_t launch_small_solve_until(hipStream_t, float *, const float *, int, int, int cap, SorParams, float, int, unsigned *result)
{
    result[0] = 0u;
    result[1] = (unsigned)cap;
    return note('x');
}
hipError_t launch_update_norm(hipStream_t, unsigned *worst, const float *, const float *, Slab, int, int, float)
{
    *worst = 0u;
    return note('x');
}
hipError_t launch_flow_stats(hipStream_t, FlowStatsRecord *out, int, const float *, const uint32_t *, int, int, int members, float, const float *)
{
    memset(out, 0, sizeof(FlowStatsRecord) * (size_t)members);
    return note('x');
}
hipError_t launch_view_scalar(hipStream_t, float *, const ViewFields &, int, float) { return note('x'); }
hipError_t launch_view_texels(hipStream_t, uint32_t *, const ViewFields &, const ViewParams &) { return note('x'); }
hipError_t launch_view_render(hipStream_t, uint16_t *, const ViewFields &, const ViewParams &, int, bool) { return note('x'); }
hipError_t launch_solid_divergence(hipStream_t, float *, float *v, const uint8_t *, int, int, float, bool zero_solids) { return note('D', zero_solids, v); }
hipError_t launch_solid_gradient(hipStream_t, float *v, const float *, const uint8_t *, int, int, float) { return note('G', 0, v); }
hipError_t launch_solid_sor(hipStream_t, float *, const float *, const float *, const uint8_t *, int, int, int, SorParams) { return note('S'); }
hipError_t launch_solid_update_norm(hipStream_t, unsigned *worst, const float *, const float *, const uint8_t *, int, int, float)
{
    *worst = 0u;
    return note('x');
}
hipError_t launch_solid_max_divergence(hipStream_t, unsigned *worst, const float *, const uint8_t *, int, int, float)
{
    *worst = 0u;
    return note('x');
}
hipError_t launch_diffuse_velocity(hipStream_t, float *, const float *u_in, const float *, const uint8_t *, int, int, int, float, float, bool zero_solids)
{
    return note('V', zero_solids, u_in);
}
// ---- the walls' (csrc/wall_kernels.h, csrc/batch.h)
hipError_t launch_wall_scatter(hipStream_t, float *v, const uint32_t *cells, const float *vel, int n) { return note('W', n, v, {nullptr, cells, vel}); }
hipError_t launch_wall_impose(hipStream_t, float *v, const uint8_t *, size_t, const uint32_t *cells, const float *vel, int n) { return note('I', n, v, {nullptr, cells, vel}); }
hipError_t launch_batch_wall_step(hipStream_t, const BatchStep &, const BatchSolids &, const BatchViscous *visc, const BatchProfile &walls, int)
{
    return note('L', visc ? 2 : 0, nullptr, walls);
}
hipError_t launch_batch_wall_step_each(hipStream_t, const BatchStep &, const BatchSolids &, const BatchViscous *visc, const BatchProfile &walls, int, const BatchMember *, float *)
{
    return note('L', visc ? 3 : 1, nullptr, walls);
}
hipError_t launch_batch_open_wall_step(hipStream_t, const BatchStep &, const BatchOpenings &o, const BatchProfile &profile, const BatchProfile &walls, int)
{
    return note('O', 0, o.codes, walls, profile);
}
hipError_t launch_batch_open_wall_step_each(hipStream_t, const BatchStep &, const BatchOpenings &o, const BatchProfile &profile, const BatchProfile &walls, int, const BatchMember *,
                                            float *)
{
    return note('O', 1, o.codes, walls, profile);
}
// ---- the openings' (csrc/batch.h, csrc/open_kernels.h)
hipError_t launch_batch_open_step(hipStream_t, const BatchStep &, const BatchOpenings &, int) { return note('o', 0); }
hipError_t launch_batch_open_step_each(hipStream_t, const BatchStep &, const BatchOpenings &, int, const BatchMember *, float *) { return note('o', 1); }
hipError_t launch_batch_open_profile_step(hipStream_t, const BatchStep &, const BatchOpenings &, const BatchProfile &, int) { return note('o', 2); }
hipError_t launch_batch_open_profile_step_each(hipStream_t, const BatchStep &, const BatchOpenings &, const BatchProfile &, int, const BatchMember *, float *) { return note('o', 3); }
hipError_t launch_batch_open_solve(hipStream_t, float *, const float *, const BatchOpenings &, int, int, int, int, SorParams) { return hipSuccess; }
hipError_t launch_batch_open_solve_each(hipStream_t, float *, const float *, const BatchOpenings &, int, int, int, const BatchMember *, float *) { return hipSuccess; }
hipError_t launch_open_velocity_stats(hipStream_t, FlowStatsRecord *, const float *, const BatchOpenings &, int, int, int, float, const float *) { return hipSuccess; }
hipError_t launch_batch_open_flux(hipStream_t, struct sfl_open_flux *, const float *, const BatchOpenings &, int, int, int, int) { return note('x'); }
hipError_t launch_open_inflow(hipStream_t, float *v, const uint32_t *, int, float, float) { return note('i', 0, v); }
hipError_t launch_open_inflow_profile(hipStream_t, float *v, const uint32_t *, const float *, int) { return note('i', 1, v); }
hipError_t launch_open_flux(hipStream_t, struct sfl_open_flux *, const float *, const uint8_t *, int, int) { return note('x'); }
hipError_t launch_open_divergence(hipStream_t, float *, float *v, const uint8_t *, const uint8_t *, int, int, float, bool zero_solids) { return note('d', zero_solids, v); }
hipError_t launch_open_gradient(hipStream_t, float *v, const float *, const uint8_t *, const uint8_t *, int, int, float) { return note('g', 0, v); }
hipError_t launch_open_sor(hipStream_t, float *, const float *, const float *, const uint8_t *, const uint8_t *, int, int, int, SorParams) { return note('s'); }
hipError_t launch_open_update_norm(hipStream_t, unsigned *worst, const float *, const float *, const uint8_t *, const uint8_t *, int, int, float)
{
    *worst = 0u;
    return note('x');
}
hipError_t launch_open_max_divergence(hipStream_t, unsigned *worst, const float *, const uint8_t *, const uint8_t *, int, int, float)
{
    *worst = 0u;
    return note('x');
}
// ---- the batches' launchers
hipError_t launch_batch_viscous_step(hipStream_t, const BatchStep &, const BatchViscous *, int) { return note('B'); }
hipError_t launch_batch_viscous_step_each(hipStream_t, const BatchStep &, const BatchViscous *, int, const BatchMember *, float *) { return note('B', 1); }
hipError_t launch_batch_viscous_solid_step(hipStream_t, const BatchStep &, const BatchSolids &, const BatchViscous *, int) { return note('B', 2); }
hipError_t launch_batch_viscous_solid_step_each(hipStream_t, const BatchStep &, const BatchSolids &, const BatchViscous *, int, const BatchMember *, float *) { return note('B', 3); }
hipError_t launch_batch_step(hipStream_t, const BatchStep &, int) { return note('x'); }
hipError_t launch_batch_step_each(hipStream_t, const BatchStep &, int, const BatchMember *, float *) { return note('x'); }
hipError_t launch_batch_step_until(hipStream_t, const BatchStep &, int, const BatchMember *, const BatchStop *, float *, int *, bool) { return note('x'); }
hipError_t launch_batch_large_step(hipStream_t, const BatchStep &, int) { return note('x'); }
hipError_t launch_batch_large_step_each(hipStream_t, const BatchStep &, int, const BatchMember *, float *) { return note('x'); }
hipError_t launch_batch_large_step_until(hipStream_t, const BatchStep &, int, const BatchMember *, const BatchStop *, float *, int *, bool) { return note('x'); }
hipError_t launch_batch_play(hipStream_t, const BatchPlay &, int, const BatchMember *, float *) { return note('x'); }
hipError_t launch_batch_solve(hipStream_t, float *, const float *, int, int, int, int, SorParams) { return hipSuccess; }
hipError_t launch_batch_solve_each(hipStream_t, float *, const float *, int, int, int, const BatchMember *, float *) { return hipSuccess; }
hipError_t launch_batch_solve_until(hipStream_t, float *, const float *, int, int, int, const BatchMember *, const BatchStop *, float *, int *) { return hipSuccess; }
hipError_t launch_batch_large_solve(hipStream_t, float *, const float *, int, int, int, int, SorParams) { return hipSuccess; }
hipError_t launch_batch_large_solve_each(hipStream_t, float *, const float *, int, int, int, const BatchMember *, float *) { return hipSuccess; }
hipError_t launch_batch_large_solve_until(hipStream_t, float *, const float *, int, int, int, const BatchMember *, const BatchStop *, float *, int *) { return hipSuccess; }
hipError_t launch_batch_solid_step(hipStream_t, const BatchStep &, const BatchSolids &, int) { return note('b'); }
hipError_t launch_batch_solid_step_each(hipStream_t, const BatchStep &, const BatchSolids &, int, const BatchMember *, float *) { return note('b', 1); }
hipError_t launch_batch_solid_solve(hipStream_t, float *, const float *, const BatchSolids &, int, int, int, int, SorParams) { return hipSuccess; }
hipError_t launch_batch_solid_solve_each(hipStream_t, float *, const float *, const BatchSolids &, int, int, int, const BatchMember *, float *) { return hipSuccess; }
hipError_t launch_solid_velocity_stats(hipStream_t, FlowStatsRecord *, const float *, const BatchSolids &, int, int, int, float, const float *) { return hipSuccess; }
hipError_t launch_batch_render(hipStream_t, uint16_t *, const uint32_t *, int, int, int, int, bool) { return hipSuccess; }
hipError_t launch_history_sample(hipStream_t, const HistorySample &, int) { return hipSuccess; }
}  // namespace sfl

static const float DT = 0.03f, DX = 0.7f, OMEGA = 1.9f, NU = 0.25f;
static bool says(const char *word) { return strstr(sfl_last_error(), word) != nullptr; }
// the log's kinds, a run of solve launches written once
static std::string kinds()
{
    std::string s;
    for (const Event &e : events)
        if (!((e.kind == 'S' || e.kind == 's') && !s.empty() && s.back() == e.kind)) s += e.kind;
    return s;
}

// ---- wall_table.h on its own ---------------------------------------------------------------------------------------------
static void the_table_builder()
{
    namespace wt = sfl::walls;
    // 4 x 3, two members: member 0 solid in row 2, member 1 solid in row 2 but for (3, 2); codes: bit 4 = fluid
    const int X = 4, Y = 3, M = 2;
    std::vector<uint8_t> codes(M * X * Y, 16);
    for (int i = 0; i < X; ++i) codes[2 * X + i] = 0;
    for (int i = 0; i < X - 1; ++i) codes[X * Y + 2 * X + i] = 0;
    const int cells[] = {3, 2, 0, 2, 1, 2, 0, 2, 1, 1};
    const float vel[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10};
    wt::Offence bad = wt::first_offence(nullptr, cells, 4, X, Y, codes.data(), false, M);
    CHECK(bad.kind == wt::Offence::kNone && bad.record < 0, "a shared mask: four records on solid cells");
    bad = wt::first_offence(nullptr, cells, 4, X, Y, codes.data(), true, M);
    CHECK(bad.kind == wt::Offence::kFluid && bad.record == 0 && bad.member == 1 && bad.i == 3 && bad.j == 2, "per-member masks: (3, 2) is fluid in member 1");
    bad = wt::first_offence(nullptr, cells, 5, X, Y, codes.data(), false, M);
    CHECK(bad.kind == wt::Offence::kFluid && bad.record == 4 && bad.member == 0, "record 4 names a fluid cell");
    const int who[] = {0, 1, 1, 0, 0};
    bad = wt::first_offence(who, cells, 4, X, Y, codes.data(), true, M);
    CHECK(bad.kind == wt::Offence::kNone, "record 0 goes to member 0 alone, where (3, 2) is solid");
    const int outside[] = {0, 2, 4, 0, 0, -1};
    bad = wt::first_offence(nullptr, outside, 3, X, Y, codes.data(), false, M);
    CHECK(bad.kind == wt::Offence::kOutside && bad.record == 1 && bad.i == 4 && bad.j == 0, "a cell outside the grid");
    // shared rows: later wins, cell order, once per member
    wt::Rows rows = wt::rows_of(nullptr, cells, vel, 4, X, M);
    CHECK(rows.size() == 1 && rows[0].size() == 3 && rows[0][0].cell == 8 && rows[0][0].u == 7 && rows[0][0].v == 8 && rows[0][1].cell == 9 &&
              rows[0][2].cell == 11 && rows[0][2].u == 1,
          "one row, three unique cells in cell order, the later record of (0, 2)");
    wt::Table t = wt::table_of(rows, M);
    CHECK(t.ok && t.offsets == std::vector<int>({0, 3, 6}) && t.cells == std::vector<uint32_t>({8, 9, 11, 8, 9, 11}) && t.vel.size() == 12 && t.vel[6] == 7 &&
              wt::records_held(rows, M) == 6,
          "a shared table counts once per member");
    // per-member rows, three members, member 1 without a record
    const int who3[] = {2, 0, 2, 0};
    rows = wt::rows_of(who3, cells, vel, 4, X, 3);
    t = wt::table_of(rows, 3);
    CHECK(rows.size() == 3 && rows[1].empty() && t.offsets == std::vector<int>({0, 1, 1, 3}) && t.cells == std::vector<uint32_t>({8, 9, 11}) && t.vel[0] == 7 &&
              t.vel[2] == 5 && t.vel[4] == 1 && wt::records_held(rows, 3) == 3,
          "CSR rows: member 0 the later record of (0, 2), member 1 empty, member 2 in cell order");
}

// ---- a batch -------------------------------------------------------------------------------------------------------------
static const int B = 3, X = 5, Y = 4, CELLS = X * Y;

static bool table_is(const sfl::BatchProfile &t, const std::vector<int> &offsets, const std::vector<uint32_t> &cells, const std::vector<float> &vel)
{
    if (!t.offsets || memcmp(t.offsets, offsets.data(), offsets.size() * sizeof(int))) return false;
    return !memcmp(t.cells, cells.data(), cells.size() * sizeof(uint32_t)) && !memcmp(t.vel, vel.data(), vel.size() * sizeof(float));
}

static void a_batch()
{
    sfl_batch *b = nullptr;
    CHECK(sfl_batch_create(&b, 0, X, Y, B) == SFL_OK && b, "create: %s", sfl_last_error());
    if (!b) return;
    int set = 5, got = 5;
    int64_t held = 5;
    const int cells[] = {4, 3, 0, 3, 2, 3, 0, 3};   // the top row; (0, 3) twice
    const float vel[] = {1, 2, 3, 4, -0.0f, 6, 7, 8};
    events.clear();
    CHECK(sfl_batch_set_wall_velocity(b, nullptr, cells, vel, 4) == SFL_ERR_STATE && says("no solids set") && !b->walls.on && !b->walls.step, "%s", sfl_last_error());
    CHECK(sfl_batch_set_wall_velocity(b, nullptr, nullptr, nullptr, 0) == SFL_OK, "clearing nothing");
    std::vector<uint8_t> mask(CELLS, 0), masks(B * CELLS, 0);
    for (int i = 0; i < X; ++i) mask[3 * X + i] = 1;
    for (int m = 0; m < B; ++m)
        for (int i = 0; i < X; ++i) masks[m * CELLS + 3 * X + i] = !(m == 1 && i == 4);   // member 1: (4, 3) is fluid
    CHECK(sfl_batch_set_solids(b, mask.data(), 0) == SFL_OK, "a shared mask: %s", sfl_last_error());
    CHECK(sfl_batch_step_n(b, 2, DT, DX, 4, OMEGA) == SFL_OK && kinds() == "bb", "without a table: the solids' step (%s)", kinds().c_str());
    // ---- a shared table
    CHECK(sfl_batch_set_wall_velocity(b, nullptr, cells, vel, 4) == SFL_OK && b->walls.on && b->walls.step && b->walls.drop, "set: %s", sfl_last_error());
    CHECK(sfl_batch_wall_velocity_info(b, &set, &held) == SFL_OK && set == 1 && held == 9, "three unique cells, once per member");
    CHECK(table_is(b->walls.table, {0, 3, 6, 9}, {15, 17, 19, 15, 17, 19, 15, 17, 19}, {7, 8, -0.0f, 6, 1, 2, 7, 8, -0.0f, 6, 1, 2, 7, 8, -0.0f, 6, 1, 2}),
          "the table as staged: rows in cell order, the later record of (0, 3), -0.0f as given");
    int ij[8];
    float uv[8];
    CHECK(sfl_batch_wall_velocity_download(b, 2, ij, uv, 4, &got) == SFL_OK && got == 3 && ij[0] == 0 && ij[1] == 3 && ij[4] == 4 && ij[5] == 3 && uv[0] == 7 &&
              signbit(uv[2]),
          "the download, in cell order");
    CHECK(sfl_batch_wall_velocity_download(b, 2, ij, uv, 2, &got) == SFL_ERR_INVALID && got == 3 && says("holds 3 records"), "%s", sfl_last_error());
    got = 5;
    CHECK(sfl_batch_wall_velocity_download(b, 2, nullptr, nullptr, 0, &got) == SFL_OK && got == 3, "no arrays and no room: the number alone, and no refusal");
    CHECK(sfl_batch_wall_velocity_download(b, 2, ij, uv, 0, &got) == SFL_ERR_INVALID, "arrays without room are refused as before");
    events.clear();
    CHECK(sfl_batch_step_n(b, 2, DT, DX, 4, OMEGA) == SFL_OK && kinds() == "LL" && events[0].n == 0 && events[0].table.cells == b->walls.table.cells,
          "with a table: the walls' step, no viscosity (%s)", kinds().c_str());
    float nu[B] = {NU, 0.0f, NU};
    sfl_member_params prm[B];
    for (int m = 0; m < B; ++m) prm[m] = sfl_member_params{DT, DX, OMEGA, 4};
    events.clear();
    CHECK(sfl_batch_set_viscosity(b, nu, 1, 3) == SFL_OK && sfl_batch_step_n(b, 1, DT, DX, 4, OMEGA) == SFL_OK && sfl_batch_step_n_each(b, 1, prm) == SFL_OK &&
              kinds() == "LL" && events[0].n == 2 && events[1].n == 3,
          "with a viscosity: the same kernels with its records (%s)", kinds().c_str());
    // ---- refusals leave the table and launch nothing
    events.clear();
    const sfl::BatchProfile before = b->walls.table;
    const int fluid[] = {0, 3, 1, 1}, outside[] = {5, 0}, member[] = {0, 3};
    const float inf[] = {1, INFINITY, 0, 0};
    CHECK(sfl_batch_set_wall_velocity(b, nullptr, fluid, vel, 2) == SFL_ERR_INVALID && says("record 1 names cell (1, 1), which is not solid in the mask"), "%s", sfl_last_error());
    CHECK(sfl_batch_set_wall_velocity(b, nullptr, outside, vel, 1) == SFL_ERR_INVALID && says("record 0 names cell (5, 0), which is not inside the grid of 5 x 4"), "%s", sfl_last_error());
    CHECK(sfl_batch_set_wall_velocity(b, member, fluid, vel, 2) == SFL_ERR_INVALID && says("record 1 names member 3"), "%s", sfl_last_error());
    CHECK(sfl_batch_set_wall_velocity(b, nullptr, cells, inf, 2) == SFL_ERR_INVALID && says("must be finite (record 0: (1, inf))"), "%s", sfl_last_error());
    CHECK(sfl_batch_set_wall_velocity(b, nullptr, cells, vel, -1) == SFL_ERR_INVALID && says("n must be >= 0"), "%s", sfl_last_error());
    CHECK(events.empty() && b->walls.on && b->walls.table.cells == before.cells && table_is(b->walls.table, {0, 3, 6, 9}, {15, 17, 19}, {7, 8}),
          "a refused call stages nothing and leaves the table as it was");
    // ---- per-member masks drop the table; a record must be solid in every member it applies to
    CHECK(sfl_batch_set_solids(b, masks.data(), 1) == SFL_OK && !b->walls.on && !b->walls.step && !b->walls.d_table, "a new mask drops the table: %s", sfl_last_error());
    CHECK(sfl_batch_wall_velocity_info(b, &set, &held) == SFL_OK && set == 0 && held == 0, "nothing held");
    events.clear();
    CHECK(sfl_batch_step_n(b, 1, DT, DX, 4, OMEGA) == SFL_OK && kinds() == "B", "the viscous step again (%s)", kinds().c_str());
    CHECK(sfl_batch_set_wall_velocity(b, nullptr, cells, vel, 4) == SFL_ERR_INVALID && says("record 0 names cell (4, 3), which is not solid in the mask of member 1"),
          "%s", sfl_last_error());
    const int who[] = {2, 0, 2, 0};
    CHECK(sfl_batch_set_wall_velocity(b, who, cells, vel, 4) == SFL_OK, "per-member records: %s", sfl_last_error());
    CHECK(table_is(b->walls.table, {0, 1, 1, 3}, {15, 17, 19}, {7, 8, -0.0f, 6, 1, 2}) && sfl_batch_wall_velocity_info(b, &set, &held) == SFL_OK && held == 3,
          "member 0 one record, member 1 none, member 2 two");
    CHECK(sfl_batch_wall_velocity_download(b, 1, nullptr, nullptr, 0, &got) == SFL_OK && got == 0, "a member without records");
    // ---- with openings: the kernels on open codes, with the wall table and the profile's table or none; the table outlives the map
    {
        std::vector<uint8_t> map(CELLS, 0);
        for (int j = 1; j < Y - 1; ++j) {
            map[j * X] = SFL_OPEN_INFLOW;
            map[j * X + X - 1] = SFL_OPEN_OUTFLOW;
        }
        const float inflow[2] = {3.5f, 0.0f};
        CHECK(sfl_batch_set_viscosity(b, nullptr, 0, 0) == SFL_OK, "the viscosity goes: openings refuse it");
        const sfl::BatchProfile held = b->walls.table;
        CHECK(sfl_batch_set_openings(b, map.data(), 0, inflow, 0) == SFL_OK && b->openings.set && b->walls.on && b->walls.table.cells == held.cells,
              "a map beside a held table: %s", sfl_last_error());
        events.clear();
        CHECK(sfl_batch_step_n(b, 1, DT, DX, 4, OMEGA) == SFL_OK && sfl_batch_step_n_each(b, 1, prm) == SFL_OK && kinds() == "OO" && events[0].n == 0 && events[1].n == 1,
              "openings and walls: the walls' step on open codes (%s; %s)", kinds().c_str(), sfl_last_error());
        for (const Event &e : events)
            CHECK(e.v == b->openings.d_codes && e.table.offsets == b->walls.table.offsets && e.table.cells == b->walls.table.cells && e.table.vel == b->walls.table.vel &&
                      !e.profile.offsets && !e.profile.cells && !e.profile.vel,
                  "the open codes, the wall table, no profile's table");
        const int pcells[] = {0, 1, 0, 2};
        const float pvel[] = {1, 0, 2, 0};
        events.clear();
        CHECK(sfl_batch_set_inflow_profile(b, nullptr, pcells, pvel, 2) == SFL_OK && sfl_batch_step_n(b, 2, DT, DX, 4, OMEGA) == SFL_OK && kinds() == "OO",
              "with a profile: %s (%s)", kinds().c_str(), sfl_last_error());
        for (const Event &e : events)
            CHECK(e.profile.offsets && e.profile.offsets == b->openings.profile_table.offsets && e.profile.cells == b->openings.profile_table.cells &&
                      e.table.cells == b->walls.table.cells && e.table.cells != e.profile.cells,
                  "the profile's table beside the walls'");
        // a refusal under openings leaves both tables; so does a cleared profile; a clear of the walls gives the openings' own step back
        events.clear();
        CHECK(sfl_batch_set_wall_velocity(b, nullptr, fluid, vel, 2) == SFL_ERR_INVALID && says("record 1 names cell (1, 1)") && events.empty() && b->walls.on &&
                  b->walls.table.cells == held.cells && table_is(b->walls.table, {0, 1, 1, 3}, {15, 17, 19}, {7, 8, -0.0f, 6, 1, 2}),
              "a refusal under openings: %s", sfl_last_error());
        CHECK(sfl_batch_set_inflow_profile(b, nullptr, nullptr, nullptr, 0) == SFL_OK && sfl_batch_step_n(b, 1, DT, DX, 4, OMEGA) == SFL_OK && kinds() == "O" &&
                  !events[0].profile.offsets,
              "the profile cleared: no table of it again (%s)", kinds().c_str());
        events.clear();
        CHECK(sfl_batch_set_wall_velocity(b, nullptr, nullptr, nullptr, 0) == SFL_OK && !b->walls.on && b->openings.set && sfl_batch_step_n(b, 1, DT, DX, 4, OMEGA) == SFL_OK &&
                  kinds() == "o",
              "the walls cleared under openings: the openings' own step (%s)", kinds().c_str());
        events.clear();
        CHECK(sfl_batch_set_wall_velocity(b, who, cells, vel, 4) == SFL_OK && sfl_batch_set_openings(b, nullptr, 0, nullptr, 0) == SFL_OK && !b->openings.set && b->walls.on &&
                  sfl_batch_step_n(b, 1, DT, DX, 4, OMEGA) == SFL_OK && kinds() == "L" && events[0].n == 0,
              "the openings cleared around a held table: the walls' step on the solids' bytes (%s; %s)", kinds().c_str(), sfl_last_error());
    }
    // ---- n == 0 clears; a cleared mask drops
    CHECK(sfl_batch_set_wall_velocity(b, nullptr, nullptr, nullptr, 0) == SFL_OK && !b->walls.on && !b->walls.step, "n == 0 clears");
    CHECK(sfl_batch_set_wall_velocity(b, who, cells, vel, 4) == SFL_OK && sfl_batch_set_solids(b, nullptr, 0) == SFL_OK && !b->walls.on && !b->walls.d_table,
          "clearing the mask drops the table");
    CHECK(sfl_batch_set_solids(b, mask.data(), 0) == SFL_OK && sfl_batch_set_wall_velocity(b, nullptr, cells, vel, 4) == SFL_OK, "set again: %s", sfl_last_error());
    sfl_batch_destroy(b);   // (with a table held: the destroy path frees it)
}

// ---- a context -----------------------------------------------------------------------------------------------------------
static void a_context(int dim_x, int dim_y)
{
    sfl_context *c = nullptr;
    CHECK(sfl_create(&c, 0, dim_x, dim_y) == SFL_OK && c, "create %d x %d: %s", dim_x, dim_y, sfl_last_error());
    if (!c) return;
    const size_t cells = (size_t)dim_x * dim_y;
    const int top = dim_y - 1, iters = 12;
    const int ij[] = {dim_x - 1, top, 0, top, 2, top, 0, top};
    const float vel[] = {1, 2, 3, 4, -0.0f, 6, 7, 8};
    int n = 5;
    CHECK(sfl_set_wall_velocity(c, ij, vel, 4) == SFL_ERR_STATE && says("no solids set") && !c->walls.on, "%s", sfl_last_error());
    std::vector<uint8_t> mask(cells, 0);
    for (int i = 0; i < dim_x; ++i) mask[(size_t)top * dim_x + i] = 1;
    CHECK(sfl_set_solids(c, mask.data()) == SFL_OK, "a lid: %s", sfl_last_error());
    events.clear();
    CHECK(sfl_step(c, DT, DX, iters, OMEGA) == SFL_OK && kinds() == "aDSGc", "the solids' step: %s", kinds().c_str());
    CHECK(sfl_set_wall_velocity(c, ij, vel, 4) == SFL_OK && c->walls.on && c->walls.step && sfl_wall_velocity_info(c, &n) == SFL_OK && n == 3, "set: %s", sfl_last_error());
    const uint32_t base = (uint32_t)top * dim_x;
    const uint32_t want_cells[] = {base, base + 2, base + (uint32_t)dim_x - 1};
    const float want_vel[] = {7, 8, -0.0f, 6, 1, 2};
    CHECK(!memcmp(c->walls.d_cells, want_cells, sizeof want_cells) && !memcmp(c->walls.d_vel, want_vel, sizeof want_vel), "the compact list: cell order, the later record");
    // ---- without a viscosity: the step that would have run, the scatter behind it
    events.clear();
    CHECK(sfl_step(c, DT, DX, iters, OMEGA) == SFL_OK && kinds() == "aDSGcW", "a step with walls: %s (%s)", kinds().c_str(), sfl_last_error());
    CHECK(events.back().n == 3 && events.back().v == c->vel && events.back().table.cells == c->walls.d_cells && events[1].n == 1, "the scatter: three records into the velocity held");
    const int fc[2] = {1, 1};
    const float fv[2] = {1, 2};
    events.clear();
    CHECK(sfl_queue_forces_at(c, 1, fc, fv, 1) == SFL_OK && sfl_step_n(c, 3, DT, DX, iters, OMEGA) == SFL_OK && kinds() == "aDSGcWafDSGcWaDSGcW",
          "step_n is n such steps: %s", kinds().c_str());
    // ---- with a viscosity: the launch over the code bytes in front of a diffusion that does not zero
    events.clear();
    CHECK(sfl_set_viscosity(c, NU, sfl::diffuse::kD + 1) == SFL_OK && sfl_step(c, DT, DX, iters, OMEGA) == SFL_OK && kinds() == "aIVVDSGcW",
          "a viscous step with walls: %s (%s)", kinds().c_str(), sfl_last_error());
    for (size_t k = 0; k < events.size(); ++k) {
        const Event &e = events[k];
        if (e.kind == 'I') CHECK(e.n == 3 && e.v == events[k + 1].v, "the diffusion reads what the launch over the code bytes wrote");
        if (e.kind == 'V') CHECK(e.n == 0, "the diffusion does not zero the solids");
        if (e.kind == 'D') CHECK(e.n == 0, "nor does the divergence");
        if (e.kind == 'W') CHECK(e.v == c->vel && e.v == events[k - 2].v, "the scatter goes where the gradient went");
    }
    events.clear();
    CHECK(sfl_diffuse_velocity(c, NU, DT, DX, 2) == SFL_OK && kinds() == "V", "the operator of its own is unchanged: %s", kinds().c_str());
    // ---- with openings: the openings' step behind the pointer the solids' step was behind, the scatter behind it
    {
        std::vector<uint8_t> map(cells, 0);
        for (int j = 1; j < dim_y - 1; ++j) {
            map[(size_t)j * dim_x] = SFL_OPEN_INFLOW;
            map[(size_t)j * dim_x + dim_x - 1] = SFL_OPEN_OUTFLOW;
        }
        const uint32_t *held = c->walls.d_cells;
        CHECK(sfl_set_viscosity(c, 0.0f, 0) == SFL_OK && sfl_set_openings(c, map.data(), 3.5f, 0.0f) == SFL_OK && c->openings.set && c->walls.on && c->walls.step &&
                  c->walls.d_cells == held,
              "a map beside a held table: %s", sfl_last_error());
        events.clear();
        CHECK(sfl_step(c, DT, DX, iters, OMEGA) == SFL_OK && kinds() == "aidsgcW", "a step with openings and walls: %s (%s)", kinds().c_str(), sfl_last_error());
        CHECK(events[1].n == 0 && events[2].n == 1 && events.back().n == 3 && events.back().v == c->vel && events.back().v == events[events.size() - 3].v &&
                  events.back().table.cells == c->walls.d_cells,
              "the uniform inflow, the divergence zeroes the solids, the scatter goes where the gradient went");
        const int pc[] = {0, 1}, bad[] = {0, top, 1, 1};
        const float pv[] = {1, 0};
        events.clear();
        CHECK(sfl_set_inflow_profile(c, pc, pv, 1) == SFL_OK && sfl_step_n(c, 2, DT, DX, iters, OMEGA) == SFL_OK && kinds() == "aidsgcWaidsgcW" && events[1].n == 1,
              "with a profile, two steps: %s (%s)", kinds().c_str(), sfl_last_error());
        events.clear();
        CHECK(sfl_set_wall_velocity(c, bad, vel, 2) == SFL_ERR_INVALID && says("record 1 names cell (1, 1)") && events.empty() && c->walls.on && c->walls.d_cells == held &&
                  !memcmp(c->walls.d_cells, want_cells, sizeof want_cells) && !memcmp(c->walls.d_vel, want_vel, sizeof want_vel),
              "a refusal under openings leaves the table: %s", sfl_last_error());
        CHECK(sfl_set_wall_velocity(c, nullptr, nullptr, 0) == SFL_OK && !c->walls.on && c->openings.set && sfl_step(c, DT, DX, iters, OMEGA) == SFL_OK && kinds() == "aidsgc",
              "the walls cleared under openings: the openings' own step (%s)", kinds().c_str());
        events.clear();
        CHECK(sfl_set_wall_velocity(c, ij, vel, 4) == SFL_OK && sfl_set_openings(c, nullptr, 0.0f, 0.0f) == SFL_OK && !c->openings.set && c->walls.on &&
                  sfl_step(c, DT, DX, iters, OMEGA) == SFL_OK && kinds() == "aDSGcW",
              "the openings cleared around a held table: the solids' step and the scatter (%s; %s)", kinds().c_str(), sfl_last_error());
        CHECK(sfl_set_viscosity(c, NU, sfl::diffuse::kD + 1) == SFL_OK, "the viscosity again: %s", sfl_last_error());
    }
    // ---- refusals leave the table
    events.clear();
    const uint32_t *before = c->walls.d_cells;
    const int fluid[] = {0, top, 1, 1}, outside[] = {dim_x, 0};
    const float nan[] = {NAN, 0};
    int out_ij[8];
    float out_uv[8];
    CHECK(sfl_set_wall_velocity(c, fluid, vel, 2) == SFL_ERR_INVALID && says("record 1 names cell (1, 1), which is not solid in the mask"), "%s", sfl_last_error());
    CHECK(sfl_set_wall_velocity(c, outside, vel, 1) == SFL_ERR_INVALID && says("which is not inside the grid"), "%s", sfl_last_error());
    CHECK(sfl_set_wall_velocity(c, ij, nan, 1) == SFL_ERR_INVALID && says("must be finite (record 0"), "%s", sfl_last_error());
    CHECK(sfl_wall_velocity_download(c, out_ij, out_uv, 2) == SFL_ERR_INVALID && says("holds 3 records"), "%s", sfl_last_error());
    CHECK(events.empty() && c->walls.on && c->walls.d_cells == before && sfl_wall_velocity_download(c, out_ij, out_uv, 4) == SFL_OK && out_ij[0] == 0 && out_ij[1] == top &&
              out_ij[4] == dim_x - 1 && out_uv[0] == 7 && signbit(out_uv[2]),
          "a refused call leaves the table as it was; the download in cell order");
    // ---- a new mask drops the table: the viscous step zeroes again
    events.clear();
    CHECK(sfl_set_solids(c, mask.data()) == SFL_OK && !c->walls.on && !c->walls.step && !c->walls.d_list && sfl_wall_velocity_info(c, &n) == SFL_OK && n == 0,
          "a new mask drops the table: %s", sfl_last_error());
    CHECK(sfl_step(c, DT, DX, iters, OMEGA) == SFL_OK && kinds() == "aVVDSGc" && events[1].n == 1, "the viscous step as before: %s", kinds().c_str());
    CHECK(sfl_set_wall_velocity(c, ij, vel, 4) == SFL_OK && sfl_set_wall_velocity(c, nullptr, nullptr, 0) == SFL_OK && !c->walls.on && !c->walls.d_list, "n == 0 clears");
    CHECK(sfl_set_wall_velocity(c, ij, vel, 4) == SFL_OK && sfl_set_solids(c, nullptr) == SFL_OK && !c->walls.on, "clearing the mask drops the table");
    CHECK(sfl_set_solids(c, mask.data()) == SFL_OK && sfl_set_wall_velocity(c, ij, vel, 4) == SFL_OK, "set again: %s", sfl_last_error());
    sfl_destroy(c);   // (with a table held: the destroy path frees it)
}

int main()
{
    the_table_builder();
    a_batch();
    a_context(6, 5);      // a small grid: the one-launch step is not taken with solids
    a_context(300, 200);
    const long left = fake_hip_live_allocations();
    printf("%d failed checks, %ld allocations left\n", failures, left);
    return failures == 0 && left == 0 ? 0 : 1;
}
