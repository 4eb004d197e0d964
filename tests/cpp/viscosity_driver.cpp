// viscosity_driver.cpp -- TEST HARNESS (tests/cpp, `make -f viscosity.mk`; tests/test_viscosity.py): the HOST side of the viscosity
// (csrc/context_viscous.cpp, csrc/viscous.cpp) and of its hooks in the step, the batches' step calls and the transports, run
// on a box without a GPU: the host units over the runtime that lives on the host (fake_hip.cpp) and kernels that do
// nothing (launch_stubs_ok.cpp).  The launchers the calls end in are stubs of THIS file that keep ONE log in the order of
// the calls, which is the order of the stream.  Two modes:
//
//   viscosity_driver               the unfused sequence of a step with a viscosity, in order, without and with solids; the
//                                  launch segmentation of the diffusion (ceil(sweeps / D) launches, the right last k, u0
//                                  the same buffer in every launch, the result made the velocity); no third buffer at
//                                  sweeps <= D; the operator of its own; every SFL_ERR_STATE refusal with its message
//                                  and nothing launched; clearing brings the old launches back, seams and the one-launch
//                                  step of a small grid included; the batches' calls; destroy leaves no allocation.
//                                  Exit status 0 and "0 failed checks".
//   viscosity_driver IN OUT        THE TILE CORE ON THE HOST: csrc/diffuse_tile.h run one workgroup's tile after the
//                                  other, thread after thread, with the launch segmentation of the host code.  IN holds
//                                  cases back to back -- int32 dim_x, dim_y, sweeps, masked; float32 nu, dt, dx; dim_y *
//                                  dim_x * 2 float32 of velocity; masked: as many mask bytes as cells -- and OUT receives
//                                  every case's velocity.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../esp32-fluid-simulation_amd/csrc/batch_state.h"
#include "../../esp32-fluid-simulation_amd/csrc/diffuse_tile.h"
#include "../../esp32-fluid-simulation_amd/csrc/history_kernels.h"
#include "../../esp32-fluid-simulation_amd/csrc/solid_kernels.h"
#include "../../esp32-fluid-simulation_amd/csrc/stats_kernels.h"
#include "../../esp32-fluid-simulation_amd/csrc/until_kernels.h"
#include "../../esp32-fluid-simulation_amd/csrc/view_kernels.h"
#include "../../esp32-fluid-simulation_amd/csrc/viscous_kernels.h"
#include "../../include/sfl.h"

extern "C" long fake_hip_live_allocations();

namespace sfl {
namespace host {
std::vector<uint8_t> solid_codes(const uint8_t *mask, int dim_x, int dim_y, size_t members);   // csrc/solids.cpp
}
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
// 'a' velocity advection, 'c' dye advection, 'A' advection + divergence in one, 'P' projection + dye advection in one,
// 'M' a step seam, 'f' forces, 'd' divergence, 'g' gradient, 'k' a launch of the plain solve, 'T' the one-launch step of a
// small grid, 't' its solve, 'D' 'S' 'G' divergence, solve launch and gradient by the solids' rule, 'V' a launch of the
// diffusion (n: its k; zero: zero_solids).  The batches': 'b' a plain or solids step launch, 'B' a viscous one (n: each |
// solids << 1), 'p' a replay of a timeline.
struct Event {
    char kind;
    int n;
    const void *in, *out, *u0, *codes;
    bool zero;
};
static std::vector<Event> events;
static hipError_t note(char kind, int n = 0, const void *in = nullptr, const void *out = nullptr, const void *u0 = nullptr,
                       const void *codes = nullptr, bool zero = false)
{
    events.push_back({kind, n, in, out, u0, codes, zero});
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
hipError_t launch_advect_divergence_tiled(hipStream_t, float *, float *, const float *, Slab, float, bool, float) { return note('A'); }
hipError_t launch_project_advect_vec3uq32(hipStream_t, uint32_t *, const uint32_t *, float *, const float *, Slab, int, int, int, int, float, bool, int *, float, int, bool *) { return note('P'); }
hipError_t launch_step_seam_tiled(hipStream_t, uint32_t *, const uint32_t *, float *, float *, const float *, const float *, Slab, float, float) { return note('M'); }
hipError_t launch_apply_forces(hipStream_t, float *, Slab, int, int, const int *, const float *, int n) { return note('f', n); }
hipError_t launch_divergence(hipStream_t, float *, const float *v, Slab, int, int, float, int) { return note('d', 0, v); }
hipError_t launch_subtract_gradient(hipStream_t, float *, const float *, Slab, int, int, float, int) { return note('g'); }
hipError_t launch_sor_half_sweep(hipStream_t, float *, const float *, Slab, int, int, int, SorParams) { return note('k'); }
hipError_t launch_sor_fused(hipStream_t, float *, const float *, const float *, Slab, SorRows, int, int, SorParams, int, int, const HaloWait *, int *senders)
{
    if (senders) *senders = 0;
    return note('k');
}
hipError_t launch_zero_rows(hipStream_t, float *, Slab, int, int) { return note('k'); }
hipError_t launch_small_step(hipStream_t, const SmallStep &) { return note('T'); }
hipError_t launch_small_solve(hipStream_t, float *, const float *, int, int, int, SorParams) { return note('t'); }
hipError_t launch_small_solve_warm(hipStream_t, float *, const float *, int, int, int, SorParams) { return note('t'); }
hipError_t launch_small_solve_until(hipStream_t, float *, const float *, int, int, int cap, SorParams, float, int, unsigned *result)
{
    result[0] = 0u;
    result[1] = (unsigned)cap;
    return note('t');
}
hipError_t launch_update_norm(hipStream_t, unsigned *worst, const float *, const float *, Slab, int, int, float)
{
    *worst = 0u;
    return note('n');
}
hipError_t launch_flow_stats(hipStream_t, FlowStatsRecord *out, int what, const float *, const uint32_t *, int, int, int members, float, const float *)
{
    memset(out, 0, sizeof(FlowStatsRecord) * (size_t)members);
    return note('s', what);
}
hipError_t launch_view_scalar(hipStream_t, float *, const ViewFields &, int, float) { return note('v'); }
hipError_t launch_view_texels(hipStream_t, uint32_t *, const ViewFields &, const ViewParams &) { return note('v'); }
hipError_t launch_view_render(hipStream_t, uint16_t *, const ViewFields &, const ViewParams &, int, bool) { return note('v'); }
// ---- by the solids' rule (csrc/solid_kernels.h)
hipError_t launch_solid_divergence(hipStream_t, float *, float *v, const uint8_t *codes, int, int, float, bool zero_solids) { return note('D', zero_solids, v, nullptr, nullptr, codes); }
hipError_t launch_solid_gradient(hipStream_t, float *, const float *, const uint8_t *codes, int, int, float) { return note('G', 0, nullptr, nullptr, nullptr, codes); }
hipError_t launch_solid_sor(hipStream_t, float *, const float *, const float *, const uint8_t *codes, int, int, int k, SorParams) { return note('S', k, nullptr, nullptr, nullptr, codes); }
hipError_t launch_solid_update_norm(hipStream_t, unsigned *worst, const float *, const float *, const uint8_t *, int, int, float)
{
    *worst = 0u;
    return note('N');
}
hipError_t launch_solid_max_divergence(hipStream_t, unsigned *worst, const float *, const uint8_t *, int, int, float)
{
    *worst = 0u;
    return note('X');
}
// ---- the viscosity's (csrc/viscous_kernels.h)
hipError_t launch_diffuse_velocity(hipStream_t, float *u_out, const float *u_in, const float *u0, const uint8_t *codes, int, int, int k, float, float, bool zero_solids)
{
    return note('V', k, u_in, u_out, u0, codes, zero_solids);
}
hipError_t launch_batch_viscous_step(hipStream_t, const BatchStep &, const BatchViscous *visc, int) { return note('B', 0, visc); }
hipError_t launch_batch_viscous_step_each(hipStream_t, const BatchStep &, const BatchViscous *visc, int, const BatchMember *, float *) { return note('B', 1, visc); }
hipError_t launch_batch_viscous_solid_step(hipStream_t, const BatchStep &, const BatchSolids &, const BatchViscous *visc, int) { return note('B', 2, visc); }
hipError_t launch_batch_viscous_solid_step_each(hipStream_t, const BatchStep &, const BatchSolids &, const BatchViscous *visc, int, const BatchMember *, float *)
{
    return note('B', 3, visc);
}
// ---- the batches' launchers
hipError_t launch_batch_step(hipStream_t, const BatchStep &, int) { return note('b'); }
hipError_t launch_batch_step_each(hipStream_t, const BatchStep &, int, const BatchMember *, float *) { return note('b', 1); }
hipError_t launch_batch_step_until(hipStream_t, const BatchStep &, int, const BatchMember *, const BatchStop *, float *, int *, bool) { return note('b', 4); }
hipError_t launch_batch_large_step(hipStream_t, const BatchStep &, int) { return note('b', 8); }
hipError_t launch_batch_large_step_each(hipStream_t, const BatchStep &, int, const BatchMember *, float *) { return note('b', 9); }
hipError_t launch_batch_large_step_until(hipStream_t, const BatchStep &, int, const BatchMember *, const BatchStop *, float *, int *, bool) { return note('b', 12); }
hipError_t launch_batch_play(hipStream_t, const BatchPlay &, int, const BatchMember *, float *) { return note('p'); }
hipError_t launch_batch_solve(hipStream_t, float *, const float *, int, int, int, int, SorParams) { return hipSuccess; }
hipError_t launch_batch_solve_each(hipStream_t, float *, const float *, int, int, int, const BatchMember *, float *) { return hipSuccess; }
hipError_t launch_batch_solve_until(hipStream_t, float *, const float *, int, int, int, const BatchMember *, const BatchStop *, float *, int *) { return hipSuccess; }
hipError_t launch_batch_large_solve(hipStream_t, float *, const float *, int, int, int, int, SorParams) { return hipSuccess; }
hipError_t launch_batch_large_solve_each(hipStream_t, float *, const float *, int, int, int, const BatchMember *, float *) { return hipSuccess; }
hipError_t launch_batch_large_solve_until(hipStream_t, float *, const float *, int, int, int, const BatchMember *, const BatchStop *, float *, int *) { return hipSuccess; }
hipError_t launch_batch_solid_step(hipStream_t, const BatchStep &, const BatchSolids &, int) { return note('b', 2); }
hipError_t launch_batch_solid_step_each(hipStream_t, const BatchStep &, const BatchSolids &, int, const BatchMember *, float *) { return note('b', 3); }
hipError_t launch_batch_solid_solve(hipStream_t, float *, const float *, const BatchSolids &, int, int, int, int, SorParams) { return hipSuccess; }
hipError_t launch_batch_solid_solve_each(hipStream_t, float *, const float *, const BatchSolids &, int, int, int, const BatchMember *, float *) { return hipSuccess; }
hipError_t launch_solid_velocity_stats(hipStream_t, FlowStatsRecord *, const float *, const BatchSolids &, int, int, int, float, const float *) { return hipSuccess; }
hipError_t launch_batch_render(hipStream_t, uint16_t *, const uint32_t *, int, int, int, int, bool) { return hipSuccess; }
hipError_t launch_history_sample(hipStream_t, const HistorySample &, int) { return hipSuccess; }
}  // namespace sfl

static const float DT = 0.03f, DX = 0.7f, OMEGA = 1.9f, NU = 0.25f;
static const int D = sfl::diffuse::kD;
static bool says(const char *word) { return strstr(sfl_last_error(), word) != nullptr; }
// the log's kinds, a run of solve launches ('k' or 'S') written once
static std::string kinds()
{
    std::string s;
    for (const Event &e : events)
        if (!((e.kind == 'k' || e.kind == 'S') && !s.empty() && s.back() == e.kind)) s += e.kind;
    return s;
}
static std::string sweep_ks()
{
    std::string s;
    for (const Event &e : events)
        if (e.kind == 'V') s += (char)('0' + e.n);
    return s;
}
static std::string ks_of(int sweeps)
{
    std::string s;
    for (int left = sweeps; left > 0; left -= D) s += (char)('0' + (left < D ? left : D));
    return s;
}
static bool info_is(sfl_context *c, float nu, int sweeps)
{
    float n = -1;
    int s = -1;
    return sfl_viscosity_info(c, &n, &s) == SFL_OK && n == nu && s == sweeps;
}

static void refusals_without_handles()
{
    float nu = 5;
    int s = 5, p = 5, q = 5;
    CHECK(sfl_set_viscosity(nullptr, NU, 2) == SFL_ERR_INVALID && says("sfl_set_viscosity: ctx is NULL"), "%s", sfl_last_error());
    CHECK(sfl_viscosity_info(nullptr, &nu, &s) == SFL_ERR_INVALID && says("sfl_viscosity_info: ctx is NULL") && nu == 5 && s == 5, "%s", sfl_last_error());
    CHECK(sfl_diffuse_velocity(nullptr, NU, DT, DX, 2) == SFL_ERR_INVALID && says("sfl_diffuse_velocity: ctx is NULL"), "%s", sfl_last_error());
    CHECK(sfl_batch_set_viscosity(nullptr, &nu, 0, 2) == SFL_ERR_INVALID && says("sfl_batch_set_viscosity: batch is NULL"), "%s", sfl_last_error());
    CHECK(sfl_batch_viscosity_info(nullptr, &s, &p, &q) == SFL_ERR_INVALID && says("sfl_batch_viscosity_info: batch is NULL") && s == 5, "%s", sfl_last_error());
    CHECK(sfl_batch_viscosity_download(nullptr, 0, 1, &nu, 4) == SFL_ERR_INVALID && says("sfl_batch_viscosity_download: batch is NULL"), "%s", sfl_last_error());
    CHECK(events.empty(), "a refused call launches nothing");
}

static void one_shape(int dim_x, int dim_y, bool small)
{
    sfl_context *c = nullptr;
    CHECK(sfl_create(&c, 0, dim_x, dim_y) == SFL_OK && c, "create %d x %d: %s", dim_x, dim_y, sfl_last_error());
    if (!c) return;
    const size_t cells = (size_t)dim_x * dim_y;
    const int iters = 12;
    const std::string solve = small ? "t" : "k";
    // ---- without a viscosity: the old launchers
    CHECK(info_is(c, 0.0f, 0) && !c->viscosity.step && !c->viscosity.set, "no viscosity at first");
    events.clear();
    CHECK(sfl_step_n(c, 3, DT, DX, iters, OMEGA) == SFL_OK, "plain steps: %s", sfl_last_error());
    const std::string plain_steps = kinds();
    CHECK(plain_steps.find('V') == std::string::npos && (small ? plain_steps == "TTT" : plain_steps.find('M') != std::string::npos), "plain: %s", plain_steps.c_str());
    // ---- the numbers' checks, each with its own message, nothing set
    CHECK(sfl_set_viscosity(c, -1.0f, 2) == SFL_ERR_INVALID && says("sfl_set_viscosity: nu must be >= 0") && info_is(c, 0.0f, 0), "%s", sfl_last_error());
    CHECK(sfl_set_viscosity(c, NAN, 2) == SFL_ERR_INVALID && says("nu must be >= 0 and not a NaN"), "%s", sfl_last_error());
    CHECK(sfl_set_viscosity(c, NU, -1) == SFL_ERR_INVALID && says("sfl_set_viscosity: sweeps must be >= 0 (got -1)") && !c->viscosity.step, "%s", sfl_last_error());
    CHECK(sfl_diffuse_velocity(c, -1.0f, DT, DX, 2) == SFL_ERR_INVALID && says("sfl_diffuse_velocity: nu must be >= 0"), "%s", sfl_last_error());
    CHECK(sfl_diffuse_velocity(c, NU, DT, DX, -3) == SFL_ERR_INVALID && says("sfl_diffuse_velocity: sweeps must be >= 0 (got -3)"), "%s", sfl_last_error());
    // ---- set: the unfused sequence, in order; sweeps <= D allocate no third buffer
    events.clear();
    CHECK(sfl_set_viscosity(c, NU, D) == SFL_OK && info_is(c, NU, D) && c->viscosity.step && events.empty(), "set: %s", sfl_last_error());
    const float *vel_before = nullptr;
    CHECK(sfl_step(c, DT, DX, iters, OMEGA) == SFL_OK && kinds() == "aVd" + solve + "gc", "a viscous step: %s (%s)", kinds().c_str(), sfl_last_error());
    for (const Event &e : events)
        if (e.kind == 'V') {
            CHECK(e.n == D && e.in == e.u0 && e.out != e.in && e.out == c->vel && !e.codes && !e.zero, "one launch: in = u0, out becomes the velocity");
            vel_before = (const float *)e.out;
        }
        else if (e.kind == 'd')
            CHECK(e.in == vel_before, "the divergence reads what the diffusion wrote");
    CHECK(!c->viscosity.d_third, "sweeps <= D: no third buffer");
    const int fc[4] = {1, 1, 0, 0};
    const float fv[4] = {1, 2, 3, 4};
    events.clear();
    CHECK(sfl_queue_forces_at(c, 1, fc, fv, 2) == SFL_OK && sfl_step_n(c, 3, DT, DX, iters, OMEGA) == SFL_OK &&
              kinds() == "aVd" + solve + "gc" + "afVd" + solve + "gc" + "aVd" + solve + "gc",
          "viscous steps with a timeline: no seams, no fused kernels, no one-launch step: %s", kinds().c_str());
    // ---- more than D sweeps: ceil(sweeps / D) launches, u0 the same buffer in all of them, the third buffer
    for (int sweeps : {1, D - 1, D, D + 1, 2 * D + 3}) {
        float *vel = c->vel;
        events.clear();
        CHECK(sfl_diffuse_velocity(c, NU, DT, DX, sweeps) == SFL_OK && kinds() == std::string(ks_of(sweeps).size(), 'V') && sweep_ks() == ks_of(sweeps),
              "the operator, %d sweeps: %s with k %s (%s)", sweeps, kinds().c_str(), sweep_ks().c_str(), sfl_last_error());
        const void *at = vel;
        for (const Event &e : events) {
            CHECK(e.u0 == vel && e.in == at && e.out != e.in && e.out != e.u0 && !e.zero, "%d sweeps: u0 / in / out of a launch", sweeps);
            at = e.out;
        }
        CHECK(c->vel == at && c->vel != vel && c->vel_tmp != c->vel && c->viscosity.d_third != c->vel && c->viscosity.d_third != c->vel_tmp,
              "%d sweeps: the last launch's buffer is the velocity, three different buffers", sweeps);
        CHECK((c->viscosity.d_third != nullptr) == (sweeps > D), "%d sweeps: the third buffer only from D + 1 on (the counts rise)", sweeps);
    }
    events.clear();
    CHECK(sfl_diffuse_velocity(c, 0.0f, DT, DX, 3) == SFL_OK && sfl_diffuse_velocity(c, NU, DT, DX, 0) == SFL_OK && events.empty(), "nu == 0 or sweeps == 0 launch nothing");
    // ---- with solids: the diffusion's first launch zeroes, the later operators are the solids'
    std::vector<uint8_t> mask(cells, 0);
    mask[cells / 2] = 1;
    events.clear();
    CHECK(sfl_set_viscosity(c, NU, D + 1) == SFL_OK && sfl_set_solids(c, mask.data()) == SFL_OK && sfl_step(c, DT, DX, iters, OMEGA) == SFL_OK && kinds() == "aVVDSGc",
          "a viscous step with solids: %s (%s)", kinds().c_str(), sfl_last_error());
    for (const Event &e : events) {
        if (e.kind == 'V') CHECK(e.zero && e.codes == c->solids.d_codes, "the diffusion knows the solids and zeroes them");
        if (e.kind == 'D') CHECK(e.n == 0 && e.in == c->vel, "the divergence by the solids' rule, nothing left to zero");
    }
    events.clear();
    CHECK(sfl_diffuse_velocity(c, NU, DT, DX, 1) == SFL_OK && events.size() == 1 && events[0].kind == 'V' && !events[0].zero && events[0].codes == c->solids.d_codes,
          "the operator honours the solids and zeroes nothing");
    CHECK(sfl_set_solids(c, nullptr) == SFL_OK, "solids cleared");
    // ---- refused while set: transports and groups, each with its own message, nothing launched
    events.clear();
    uint8_t id[256] = {};
    CHECK(sfl_comm_attach(c, id, 4) == SFL_ERR_INVALID, "attach: its arguments first");
    CHECK(sfl_comm_attach(c, id, sizeof id) == SFL_ERR_STATE && says("a viscosity set") && says("a transport") && !c->transport, "attach: %s", sfl_last_error());
    CHECK(sfl_comm_emulate(c) == SFL_ERR_STATE && says("a viscosity set"), "emulate: %s", sfl_last_error());
    CHECK(sfl_comm_emulate_rccl(c) == SFL_ERR_STATE && says("a viscosity set"), "emulate_rccl: %s", sfl_last_error());
    CHECK(sfl_group_link(&c, 1) == SFL_ERR_STATE && says("a viscosity set") && says("a group") && !c->group, "link: %s", sfl_last_error());
    CHECK(events.empty(), "a refused attach launches nothing");
    // ---- cleared, either way: the old launches again, seams and the small grid's step included
    CHECK(sfl_set_viscosity(c, 0.0f, 5) == SFL_OK && info_is(c, 0.0f, 0) && !c->viscosity.step, "nu == 0 clears");
    events.clear();
    CHECK(sfl_step_n(c, 3, DT, DX, iters, OMEGA) == SFL_OK && kinds() == plain_steps, "cleared steps: %s, at first %s", kinds().c_str(), plain_steps.c_str());
    CHECK(sfl_set_viscosity(c, NU, 2) == SFL_OK && c->viscosity.step && sfl_set_viscosity(c, NU, 0) == SFL_OK && !c->viscosity.step && !c->viscosity.set, "sweeps == 0 clears");
    events.clear();
    CHECK(sfl_step_n(c, 3, DT, DX, iters, OMEGA) == SFL_OK && kinds() == plain_steps, "cleared again: %s", kinds().c_str());
    // ---- destroy with a viscosity set and the third buffer held
    CHECK(sfl_set_viscosity(c, NU, 2 * D) == SFL_OK && c->viscosity.d_third && sfl_destroy(c) == SFL_OK, "destroy with a viscosity set");
    events.clear();
}

static void slabs_and_transports()
{
    sfl_context *slab = nullptr, *hand = nullptr;
    CHECK(sfl_create_slab(&slab, 0, 64, 512, 0, 2) == SFL_OK && slab, "slab: %s", sfl_last_error());
    CHECK(sfl_set_viscosity(slab, NU, 2) == SFL_ERR_STATE && says("sfl_set_viscosity") && says("whole-domain contexts only (slab 0/2)") && says("nothing set") && !slab->viscosity.set,
          "a slab: %s", sfl_last_error());
    CHECK(sfl_diffuse_velocity(slab, NU, DT, DX, 2) == SFL_ERR_STATE && says("sfl_diffuse_velocity") && says("slab 0/2") && says("nothing launched"), "a slab's operator: %s", sfl_last_error());
    CHECK(sfl_set_viscosity(slab, 0.0f, 0) == SFL_OK && sfl_diffuse_velocity(slab, 0.0f, DT, DX, 2) == SFL_OK, "clearing and nu == 0 are always let through");
    CHECK(sfl_create(&hand, 0, 9, 7) == SFL_OK && hand && sfl_group_link(&hand, 1) == SFL_OK && hand->transport, "a group of one: %s", sfl_last_error());
    CHECK(sfl_set_viscosity(hand, NU, 2) == SFL_ERR_STATE && says("transport attached") && says("nothing set") && !hand->viscosity.step, "a context with a transport: %s", sfl_last_error());
    CHECK(sfl_diffuse_velocity(hand, NU, DT, DX, 2) == SFL_ERR_STATE && says("transport attached") && says("nothing launched"), "... its operator: %s", sfl_last_error());
    CHECK(events.empty(), "refusals launch nothing");
    CHECK(sfl_destroy(hand) == SFL_OK && sfl_destroy(slab) == SFL_OK, "destroy");
    events.clear();
}

static void batches()
{
    const int B = 3, X = 9, Y = 7;
    sfl_batch *b = nullptr, *large = nullptr;
    CHECK(sfl_batch_create(&b, 0, X, Y, B) == SFL_OK && b && sfl_batch_create_large(&large, 0, X, Y, B) == SFL_OK && large, "create: %s", sfl_last_error());
    if (!b || !large) return;
    float nu[B] = {0.0f, 0.5f, 2.0f}, got[B] = {9, 9, 9};
    const float bad[B] = {0.0f, 0.5f, -2.0f}, nan_[B] = {0.0f, NAN, -2.0f};
    int set = -1, per = -1, sweeps = -1;
    sfl_member_params prm[B];
    sfl_member_stop stop[B];
    for (int m = 0; m < B; ++m) {
        prm[m] = sfl_member_params{DT, DX + 0.1f * m, OMEGA, 4 + m};
        stop[m] = sfl_member_stop{1e-3f, 2};
    }
    // ---- the checks, in the header's order
    CHECK(sfl_batch_set_viscosity(b, nu, 2, 2) == SFL_ERR_INVALID && says("per_member must be 0 or 1 (got 2)"), "%s", sfl_last_error());
    CHECK(sfl_batch_set_viscosity(b, nu, 1, -1) == SFL_ERR_INVALID && says("sweeps must be >= 0 (got -1)"), "%s", sfl_last_error());
    CHECK(sfl_batch_set_viscosity(b, bad, 1, 2) == SFL_ERR_INVALID && says("member 2: nu must be >= 0"), "%s", sfl_last_error());
    CHECK(sfl_batch_set_viscosity(b, nan_, 1, 2) == SFL_ERR_INVALID && says("member 1: nu must be >= 0 and not a NaN"), "%s", sfl_last_error());
    CHECK(sfl_batch_set_viscosity(b, bad, 0, 2) == SFL_OK && sfl_batch_set_viscosity(b, nullptr, 0, 0) == SFL_OK, "a shared nu reads one float");
    CHECK(sfl_batch_set_viscosity(large, bad, 1, 2) == SFL_ERR_INVALID, "a large batch: the arguments first");
    CHECK(sfl_batch_set_viscosity(large, nu, 1, 2) == SFL_ERR_STATE && says("sfl_batch_create_large") && says("no room for u0") && !large->viscosity.set, "large: %s", sfl_last_error());
    CHECK(sfl_batch_set_viscosity(large, nullptr, 0, 0) == SFL_OK, "clearing is always let through");
    CHECK(sfl_batch_viscosity_info(b, &set, &per, &sweeps) == SFL_OK && set == 0 && per == 0 && sweeps == 0, "nothing set");
    CHECK(sfl_batch_viscosity_download(b, 0, B, got, sizeof got) == SFL_OK && got[0] == 0 && got[2] == 0, "nothing set: zeros");
    // ---- plain launches
    events.clear();
    CHECK(sfl_batch_step_n(b, 2, DT, DX, 5, OMEGA) == SFL_OK && sfl_batch_step_n_each(b, 1, prm) == SFL_OK && kinds() == "bbb", "plain: %s", kinds().c_str());
    const int who[1] = {1}, at[2] = {2, 2};
    const float vel[2] = {1, 1};
    events.clear();
    CHECK(sfl_batch_queue_forces_at(b, 1, who, at, vel, 1) == SFL_OK && sfl_batch_step_n(b, 3, DT, DX, 5, OMEGA) == SFL_OK && kinds() == "p", "a plain timeline is replayed: %s", kinds().c_str());
    // ---- set: one launch per step through the viscous kernels, the table staged per call
    events.clear();
    CHECK(sfl_batch_set_viscosity(b, nu, 1, 3) == SFL_OK && events.empty() && b->viscosity.step && b->viscosity.stage, "set: %s", sfl_last_error());
    CHECK(sfl_batch_viscosity_info(b, &set, &per, &sweeps) == SFL_OK && set == 1 && per == 1 && sweeps == 3, "info");
    CHECK(sfl_batch_viscosity_download(b, 1, 2, got, 8) == SFL_OK && got[0] == 0.5f && got[1] == 2.0f, "download");
    CHECK(sfl_batch_viscosity_download(b, 1, 2, got, 12) == SFL_ERR_INVALID && says("bytes, got"), "download sizes: %s", sfl_last_error());
    CHECK(sfl_batch_viscosity_download(b, 2, 2, got, 8) == SFL_ERR_INVALID && says("not inside the batch"), "download range: %s", sfl_last_error());
    CHECK(sfl_batch_queue_forces_at(b, 1, who, at, vel, 1) == SFL_OK && sfl_batch_step_n(b, 3, DT, DX, 5, OMEGA) == SFL_OK && kinds() == "BBB" && events[0].n == 0,
          "viscous steps, a timeline is not replayed: %s (%s)", kinds().c_str(), sfl_last_error());
    const sfl::BatchViscous *table = (const sfl::BatchViscous *)b->viscosity.d_table;
    const sfl::diffuse::Coefficients k1 = sfl::diffuse::coefficients(0.5f, DT, DX);
    CHECK(table && events[0].in == table && table[0].sweeps == 0 && table[1].sweeps == 3 && table[1].a == k1.a && table[1].c == k1.c && table[2].sweeps == 3, "the table of a uniform call");
    events.clear();
    CHECK(sfl_batch_step_n_each(b, 2, prm) == SFL_OK && kinds() == "BB" && events[0].n == 1, "each: %s", kinds().c_str());
    const sfl::diffuse::Coefficients k2 = sfl::diffuse::coefficients(2.0f, DT, DX + 0.2f);
    CHECK(table[2].a == k2.a && table[2].c == k2.c && table[0].sweeps == 0, "the table of an _each call: the member's own dt and dx");
    events.clear();
    CHECK(sfl_batch_step_n_until(b, 1, prm, nullptr) == SFL_ERR_INVALID, "until: its arguments first");
    CHECK(sfl_batch_step_n_until(b, 1, prm, stop) == SFL_ERR_STATE && says("sfl_batch_step_n_until") && says("a viscosity set") && events.empty(), "until: %s", sfl_last_error());
    std::vector<uint8_t> mask((size_t)X * Y, 0);
    mask[10] = 1;
    CHECK(sfl_batch_set_solids(b, mask.data(), 0) == SFL_OK && sfl_batch_step_n(b, 1, DT, DX, 5, OMEGA) == SFL_OK && sfl_batch_step_n_each(b, 1, prm) == SFL_OK && kinds() == "BB" &&
              events[0].n == 2 && events[1].n == 3,
          "with solids: %s", kinds().c_str());
    // ---- cleared: what was launched before
    events.clear();
    CHECK(sfl_batch_set_viscosity(b, nullptr, 0, 0) == SFL_OK && !b->viscosity.step && sfl_batch_step_n(b, 1, DT, DX, 5, OMEGA) == SFL_OK && kinds() == "b" && events[0].n == 2,
          "cleared, solids still set: %s", kinds().c_str());
    events.clear();
    CHECK(sfl_batch_set_solids(b, nullptr, 0) == SFL_OK && sfl_batch_step_n_until(b, 1, prm, stop) == SFL_OK && kinds() == "b" && events[0].n == 4, "cleared: until works: %s", sfl_last_error());
    CHECK(sfl_batch_set_viscosity(b, nu, 0, 1) == SFL_OK && sfl_batch_destroy(b) == SFL_OK && sfl_batch_destroy(large) == SFL_OK, "destroy with a viscosity set");
    events.clear();
}

// ---- the tile core on the host ---------------------------------------------------------------------------------------------
static int run_tiles(const char *in_path, const char *out_path)
{
    namespace df = sfl::diffuse;
    FILE *in = fopen(in_path, "rb"), *out = fopen(out_path, "wb");
    if (!in || !out) return 2;
    std::vector<df::Cells> cells(df::kThreads);
    std::vector<df::Vec2> lds(df::kLdsCells);
    int cases = 0;
    for (;;) {
        int32_t head[4];
        float prm[3];
        if (fread(head, 4, 4, in) != 4) break;
        if (fread(prm, 4, 3, in) != 3) return 3;
        const int dim_x = head[0], dim_y = head[1], sweeps = head[2];
        const size_t n = (size_t)dim_x * dim_y;
        std::vector<df::Vec2> vel(n), tmp(n), third(n);
        std::vector<uint8_t> mask(n, 0), codes;
        if (fread(vel.data(), 8, n, in) != n) return 3;
        if (head[3]) {
            if (fread(mask.data(), 1, n, in) != n) return 3;
            codes = sfl::host::solid_codes(mask.data(), dim_x, dim_y, 1);
        }
        const df::Coefficients k = df::coefficients(prm[0], prm[1], prm[2]);
        const df::Vec2 *cur = vel.data();
        df::Vec2 *next = tmp.data(), *spare = third.data();
        for (int l = 0; l < (prm[0] == 0.0f ? 0 : df::launches_of(sweeps)); ++l) {   // the segmentation of context_viscous.cpp's diffuse
            df::Tile t;
            t.u_in = cur;
            t.u0 = vel.data();
            t.u_out = next;
            t.codes = head[3] ? codes.data() : nullptr;
            t.dim_x = dim_x;
            t.dim_y = dim_y;
            t.k = df::sweeps_of_launch(sweeps, l);
            t.a = k.a;
            t.c = k.c;
            t.zero_solids = false;
            for (int ty = 0; ty < df::tiles_y(dim_y); ++ty)
                for (int tx = 0; tx < df::tiles_x(dim_x); ++tx) {   // one workgroup: its phases, each thread after thread
                    t.x0 = tx * df::kTX;
                    t.y0 = ty * df::kTY;
                    for (int tid = 0; tid < df::kThreads; ++tid) df::load(cells[tid], lds.data(), t, tid);
                    for (int it = 0; it < t.k; ++it)
                        for (int colour = 0; colour < 2; ++colour)
                            for (int tid = 0; tid < df::kThreads; ++tid) df::half_sweep(cells[tid], lds.data(), colour, t, tid);
                    for (int tid = 0; tid < df::kThreads; ++tid) df::store(lds.data(), t, tid);
                }
            cur = next;
            std::swap(next, spare);
        }
        if (fwrite(cur, 8, n, out) != n) return 4;
        ++cases;
    }
    fclose(in);
    if (fclose(out) != 0) return 4;
    printf("viscosity driver: %d cases diffused tile by tile (TX %d, TY %d, D %d)\n", cases, df::kTX, df::kTY, df::kD);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 3) return run_tiles(argv[1], argv[2]);
    refusals_without_handles();
    one_shape(7, 5, true);
    one_shape(257, 130, false);
    slabs_and_transports();
    batches();
    const long left = fake_hip_live_allocations();
    printf("viscosity driver: %d failed checks, %ld allocations left\n", failures, left);
    return failures || left ? 1 : 0;
}
