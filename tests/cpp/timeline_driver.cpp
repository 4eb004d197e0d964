// timeline_driver.cpp -- TEST HARNESS (tests/cpp, `make -f timeline.mk`; tests/test_force_timeline.py): the timeline of queued
// forces (include/sfl.h, "the timeline rule") on the HOST side of the library, run on a box without a GPU under
// AddressSanitizer + UBSan: the host units of contexts and batches over the runtime that lives on the host (fake_hip.cpp) and
// kernels that do nothing (launch_stubs_ok.cpp).  The launchers of the batches (csrc/batch.h) are stubs of THIS file that keep a
// log: "device" memory is host memory here, so a stub reads the staged CSR table as the kernel would and notes which records
// every member would apply in every step of every launch.  What is checked: refusals queue nothing, sfl_[batch_]forces_pending
// after queueing at scattered steps, the shift across step calls of every kind, a refused step call leaves the timeline as it
// was, forget, which launch (one per step, or batch_play.hip's one per call) a call takes and the records each step gets.
// Exit status 0 and "0 failed checks" = every call did what the header says.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../esp32-fluid-simulation_amd/csrc/batch.h"
#include "../../esp32-fluid-simulation_amd/csrc/stats_kernels.h"
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

// ---- the log of the batch launchers -------------------------------------------------------------------------------------
struct Applied {
    int launch, step, member, i, j;   // step: inside the launch
    float vx;
};
struct Launch {
    char kind;   // 's' one step (uniform), 'e' each, 'u' until, 'p' play
    int steps;
    const int *offsets;
};
static std::vector<Applied> applied;
static std::vector<Launch> launches;

static void note_row(const sfl::SmallStep &s, const int *row, int batch, int step)
{
    for (int m = 0; m < batch; ++m)
        for (int f = row[m]; f < row[m + 1]; ++f)
            applied.push_back({(int)launches.size(), step, m, s.force_cells[2 * f], s.force_cells[2 * f + 1], s.force_vel[2 * f]});
}
static hipError_t note_step(char kind, const sfl::BatchStep &a, int batch)
{
    if (a.force_offsets) note_row(a.step, a.force_offsets, batch, 0);
    launches.push_back({kind, 1, a.force_offsets});
    return hipSuccess;
}

namespace sfl {
bool small_grid_fits(int dim_x, int dim_y)   // (the real rule of small_grid.hip; launch_stubs_ok.cpp's answer is "no")
{
    return dim_x >= 2 && dim_y >= 2 && (long long)dim_x * dim_y <= kSmallGridMaxCells &&
           (long long)dim_y * ((dim_x + 1) / 2) <= kSmallGridMaxCells / 2;
}
hipError_t launch_batch_step(hipStream_t, const BatchStep &a, int batch) { return note_step('s', a, batch); }
hipError_t launch_batch_step_each(hipStream_t, const BatchStep &a, int batch, const BatchMember *, float *) { return note_step('e', a, batch); }
hipError_t launch_batch_step_until(hipStream_t, const BatchStep &a, int batch, const BatchMember *, const BatchStop *, float *, int *, bool)
{
    return note_step('u', a, batch);
}
hipError_t launch_batch_large_step(hipStream_t, const BatchStep &a, int batch) { return note_step('s', a, batch); }
hipError_t launch_batch_large_step_each(hipStream_t, const BatchStep &a, int batch, const BatchMember *, float *) { return note_step('e', a, batch); }
hipError_t launch_batch_large_step_until(hipStream_t, const BatchStep &a, int batch, const BatchMember *, const BatchStop *, float *, int *, bool)
{
    return note_step('u', a, batch);
}
hipError_t launch_batch_play(hipStream_t, const BatchPlay &a, int batch, const BatchMember *, float *)
{
    for (int k = 0; a.force_rows && k < a.rows; ++k) note_row(a.step, a.force_rows + (size_t)k * batch, batch, k);
    launches.push_back({'p', a.steps, a.force_rows});
    return hipSuccess;
}
hipError_t launch_batch_solve(hipStream_t, float *, const float *, int, int, int, int, SorParams) { return hipSuccess; }
hipError_t launch_batch_solve_each(hipStream_t, float *, const float *, int, int, int, const BatchMember *, float *) { return hipSuccess; }
hipError_t launch_batch_solve_until(hipStream_t, float *, const float *, int, int, int, const BatchMember *, const BatchStop *, float *, int *)
{
    return hipSuccess;
}
hipError_t launch_batch_large_solve(hipStream_t, float *, const float *, int, int, int, int, SorParams) { return hipSuccess; }
hipError_t launch_batch_large_solve_each(hipStream_t, float *, const float *, int, int, int, const BatchMember *, float *) { return hipSuccess; }
hipError_t launch_batch_large_solve_until(hipStream_t, float *, const float *, int, int, int, const BatchMember *, const BatchStop *, float *, int *)
{
    return hipSuccess;
}
hipError_t launch_batch_render(hipStream_t, uint16_t *, const uint32_t *, int, int, int, int, bool) { return hipSuccess; }
hipError_t launch_flow_stats(hipStream_t, FlowStatsRecord *, int, const float *, const uint32_t *, int, int, int, float, const float *)
{
    return hipSuccess;
}
}  // namespace sfl

static bool pending_is(sfl_context *c, int records, int last)
{
    int r = -7, l = -7;
    return sfl_forces_pending(c, &r, &l) == SFL_OK && r == records && l == last;
}
static bool pending_is(sfl_batch *b, int records, int last)
{
    int r = -7, l = -7;
    return sfl_batch_forces_pending(b, &r, &l) == SFL_OK && r == records && l == last;
}

static const int kCells[8] = {1, 1, 2, 3, 1, 1, 99, 99};
static const float kVel[8] = {1.f, 0.f, 2.f, 0.f, 3.f, 0.f, 4.f, 0.f};
static const float DT = 0.03f, DX = 1.0f, OMEGA = 1.9f;

static void contexts(int dim_x, int dim_y)
{
    sfl_context *c = nullptr;
    CHECK(sfl_create(&c, 0, dim_x, dim_y) == SFL_OK && c, "create: %s", sfl_last_error());
    if (!c) return;
    // refusals queue nothing
    CHECK(sfl_queue_forces_at(nullptr, 0, kCells, kVel, 1) == SFL_ERR_INVALID, "NULL ctx");
    CHECK(sfl_queue_forces_at(c, -1, kCells, kVel, 1) == SFL_ERR_INVALID && strstr(sfl_last_error(), "step"), "step < 0: %s", sfl_last_error());
    CHECK(sfl_queue_forces_at(c, 2, nullptr, kVel, 1) == SFL_ERR_INVALID && sfl_queue_forces_at(c, 2, kCells, nullptr, 1) == SFL_ERR_INVALID, "NULL arrays");
    const sfl_drag inside = {3, 2, 1.f, 2.f}, outside = {(uint16_t)dim_y, 0, 1.f, 2.f};
    const sfl_drag two[2] = {inside, outside};
    CHECK(sfl_queue_drags_at(c, 3, two, 2) == SFL_ERR_INVALID && strstr(sfl_last_error(), "drag 1"), "a drag outside the domain: %s", sfl_last_error());
    CHECK(sfl_queue_drags_at(c, -2, &inside, 1) == SFL_ERR_INVALID && sfl_queue_drags_at(c, 1, nullptr, 1) == SFL_ERR_INVALID, "drags: step < 0, NULL");
    CHECK(pending_is(c, 0, -1), "the refused calls queued nothing");
    CHECK(sfl_forces_pending(nullptr, nullptr, nullptr) == SFL_ERR_INVALID && sfl_forget_forces(nullptr) == SFL_ERR_INVALID, "NULL ctx");
    CHECK(sfl_forces_pending(c, nullptr, nullptr) == SFL_OK, "both out pointers may be NULL");
    // steps {0, 3, 3, 7}: one by the old call, one by a drag
    CHECK(sfl_queue_forces(c, kCells, kVel, 1) == SFL_OK && sfl_queue_forces_at(c, 3, kCells + 2, kVel + 2, 1) == SFL_OK &&
              sfl_queue_drags_at(c, 3, &inside, 1) == SFL_OK && sfl_queue_forces_at(c, 7, kCells + 4, kVel + 4, 1) == SFL_OK, "queue: %s", sfl_last_error());
    CHECK(pending_is(c, 4, 7), "4 records, the last at step 7");
    CHECK(sfl_queue_forces_at(c, 9, kCells, kVel, 0) == SFL_OK && pending_is(c, 4, 7), "n == 0 queues nothing");
    // neither a solve nor an upload consumes or shifts; refused step calls neither
    std::vector<float> d((size_t)dim_x * dim_y, 0.5f);
    CHECK(sfl_upload(c, SFL_FIELD_DIVERGENCE, d.data(), d.size() * 4) == SFL_OK && sfl_poisson_solve(c, DX, 3, OMEGA) == SFL_OK, "solve: %s", sfl_last_error());
    CHECK(sfl_step_n(c, -1, DT, DX, 3, OMEGA) == SFL_ERR_INVALID && sfl_step_n(c, 2, DT, DX, -3, OMEGA) == SFL_ERR_INVALID &&
              sfl_step(c, DT, DX, -3, OMEGA) == SFL_ERR_INVALID && sfl_step_n(c, 0, DT, DX, 3, OMEGA) == SFL_OK, "refused step calls, n == 0");
    CHECK(pending_is(c, 4, 7), "... leave the timeline as it was");
    // the shift across two step calls
    CHECK(sfl_step(c, DT, DX, 3, OMEGA) == SFL_OK && pending_is(c, 3, 6), "sfl_step consumes step 0: %s", sfl_last_error());
    CHECK(sfl_step_n(c, 3, DT, DX, 3, OMEGA) == SFL_OK && pending_is(c, 1, 3), "sfl_step_n(3) consumes [0, 3): %s", sfl_last_error());
    CHECK(sfl_queue_forces(c, kCells, kVel, 2) == SFL_OK && pending_is(c, 3, 3), "step 0 again");
    CHECK(sfl_forget_forces(c) == SFL_OK && pending_is(c, 0, -1), "forget");
    CHECK(sfl_step_n(c, 5, DT, DX, 3, OMEGA) == SFL_OK && pending_is(c, 0, -1), "steps on an empty timeline");
    CHECK(sfl_destroy(c) == SFL_OK, "destroy");
}

// two virtual ranks: a record queued on one rank is every rank's, and a step of the group shifts every rank's timeline
static void linked_ranks()
{
    sfl_context *r[2] = {nullptr, nullptr};
    CHECK(sfl_create_slab(&r[0], 0, 160, 128, 0, 2) == SFL_OK && sfl_create_slab(&r[1], 0, 160, 128, 1, 2) == SFL_OK, "slabs: %s", sfl_last_error());
    if (!r[0] || !r[1]) return;
    CHECK(sfl_group_link(r, 2) == SFL_OK, "link: %s", sfl_last_error());
    CHECK(sfl_queue_forces_at(r[0], 2, kCells, kVel, 2) == SFL_OK && sfl_queue_forces_at(r[1], 0, kCells, kVel, 1) == SFL_OK, "queue");
    CHECK(pending_is(r[0], 3, 2) && pending_is(r[1], 3, 2), "both ranks hold the same timeline");
    CHECK(sfl_step_n(r[0], 2, DT, DX, 4, OMEGA) == SFL_OK, "step_n: %s", sfl_last_error());
    CHECK(pending_is(r[0], 2, 0) && pending_is(r[1], 2, 0), "both ranks' timelines moved down by 2");
    CHECK(sfl_forget_forces(r[1]) == SFL_OK && pending_is(r[0], 0, -1) && pending_is(r[1], 0, -1), "forget on one rank forgets on all");
    CHECK(sfl_destroy(r[0]) == SFL_OK && sfl_destroy(r[1]) == SFL_OK, "destroy");
}

// the records of launch l, step s as "member:i:vx" in the order a member's workgroup would apply them
static std::vector<Applied> of(int launch, int step)
{
    std::vector<Applied> r;
    for (const Applied &a : applied)
        if (a.launch == launch && a.step == step) r.push_back(a);
    return r;
}

static void batches(bool large)
{
    const int B = 3;
    sfl_batch *b = nullptr;
    CHECK((large ? sfl_batch_create_large : sfl_batch_create)(&b, 0, 8, 6, B) == SFL_OK && b, "create: %s", sfl_last_error());
    if (!b) return;
    const int m0[1] = {0}, m2[1] = {2}, bad[2] = {1, 3}, m22[2] = {2, 2};
    CHECK(sfl_batch_queue_forces_at(nullptr, 0, m0, kCells, kVel, 1) == SFL_ERR_INVALID, "NULL batch");
    CHECK(sfl_batch_queue_forces_at(b, -1, m0, kCells, kVel, 1) == SFL_ERR_INVALID && strstr(sfl_last_error(), "step"), "step < 0");
    CHECK(sfl_batch_queue_forces_at(b, 1, bad, kCells, kVel, 2) == SFL_ERR_INVALID && strstr(sfl_last_error(), "force 1 names member 3"), "member outside: %s", sfl_last_error());
    CHECK(sfl_batch_queue_forces_at(b, 1, nullptr, kCells, kVel, 1) == SFL_ERR_INVALID && sfl_batch_queue_forces_at(b, 1, m0, nullptr, kVel, 1) == SFL_ERR_INVALID &&
              sfl_batch_queue_forces_at(b, 1, m0, kCells, nullptr, 1) == SFL_ERR_INVALID, "NULL arrays");
    CHECK(pending_is(b, 0, -1), "the refused calls queued nothing");
    CHECK(sfl_batch_forces_pending(nullptr, nullptr, nullptr) == SFL_ERR_INVALID && sfl_batch_forget_forces(nullptr) == SFL_ERR_INVALID, "NULL batch");

    // ---- one launch per step: steps {0, 3, 3, 7}; the two of step 3 hit one cell of member 2 (the later must come later) and
    //      a cell outside the domain rides along (skipped by the kernel, not by the host)
    applied.clear();
    launches.clear();
    const int cell11[4] = {1, 1, 1, 1};
    const float first_then_second[4] = {5.f, 0.f, 6.f, 0.f};
    CHECK(sfl_batch_queue_forces(b, m0, kCells, kVel, 1) == SFL_OK && sfl_batch_queue_forces_at(b, 3, m22, cell11, first_then_second, 2) == SFL_OK &&
              sfl_batch_queue_forces_at(b, 7, m2, kCells + 6, kVel + 6, 1) == SFL_OK, "queue: %s", sfl_last_error());
    CHECK(pending_is(b, 4, 7), "4 records, the last at step 7");
    sfl_member_params prm[B];
    sfl_member_stop stop[B];
    for (int m = 0; m < B; ++m) {
        prm[m] = {DT, DX, OMEGA, 3 + m};
        stop[m] = {-1.0f, 2};
    }
    CHECK(sfl_batch_poisson_solve(b, DX, 3, OMEGA) == SFL_OK && pending_is(b, 4, 7), "a solve neither consumes nor shifts");
    CHECK(sfl_batch_step_n(b, -1, DT, DX, 3, OMEGA) == SFL_ERR_INVALID && sfl_batch_step_n(b, 2, DT, DX, -1, OMEGA) == SFL_ERR_INVALID &&
              sfl_batch_step_n_each(b, 2, nullptr) == SFL_ERR_INVALID && sfl_batch_step_n(b, 0, DT, DX, 3, OMEGA) == SFL_OK, "refused calls, n == 0");
    CHECK(pending_is(b, 4, 7) && launches.empty(), "... leave the timeline as it was");
    CHECK(sfl_batch_step_n(b, 2, DT, DX, 3, OMEGA) == SFL_OK && pending_is(b, 3, 5), "step_n(2): %s", sfl_last_error());
    CHECK(launches.size() == 2 && launches[0].kind == 's' && launches[1].kind == 's', "records in step 0 only: one launch per step");
    CHECK(of(0, 0).size() == 1 && of(0, 0)[0].member == 0 && of(0, 0)[0].vx == 1.f && launches[1].offsets == nullptr, "step 0 has the record, step 1 none");
    // (the rest of the timeline is on the device since that call: rows of ONE table from here on)
    CHECK(sfl_batch_step_n_until(b, 3, prm, stop) == SFL_OK && pending_is(b, 1, 2), "step_n_until(3): %s", sfl_last_error());
    CHECK(launches.size() == 5 && launches[2].kind == 'u' && launches[2].offsets == nullptr && launches[3].offsets && launches[4].offsets == nullptr, "rows");
    {
        const std::vector<Applied> r = of(3, 0);
        CHECK(r.size() == 2 && r[0].member == 2 && r[0].vx == 5.f && r[1].member == 2 && r[1].vx == 6.f, "the two records of one cell keep their queue order");
    }
    // a recorder without room refuses the call: the timeline stays
    CHECK(sfl_batch_record_start(b, 1, 0, B, 1, 1, 1) == SFL_OK, "recorder: %s", sfl_last_error());
    CHECK(sfl_batch_step_n_each(b, 3, prm) == SFL_ERR_STATE && pending_is(b, 1, 2) && launches.size() == 5, "refused for lack of free frames: %s", sfl_last_error());
    CHECK(sfl_batch_record_stop(b) == SFL_OK, "recorder off");

    // ---- a record in some step of [1, n): ONE launch for a small batch by step_n / step_n_each, else one per step
    CHECK(sfl_batch_queue_forces_at(b, 0, m0, kCells + 2, kVel + 2, 1) == SFL_OK && pending_is(b, 2, 2), "one more at step 0");
    applied.clear();
    launches.clear();
    CHECK(sfl_batch_step_n_each(b, 4, prm) == SFL_OK && pending_is(b, 0, -1), "step_n_each(4): %s", sfl_last_error());
    if (large) {
        CHECK(launches.size() == 4 && launches[0].kind == 'e' && launches[1].offsets == nullptr && launches[3].offsets == nullptr &&
                  launches[2].offsets == launches[0].offsets + 2 * B, "a large batch: per-step launches on rows of one table");
        CHECK(of(0, 0).size() == 1 && of(0, 0)[0].vx == 2.f && of(2, 0).size() == 1 && of(2, 0)[0].member == 2 && of(2, 0)[0].i == 99, "steps 0 and 2");
    } else {
        CHECK(launches.size() == 1 && launches[0].kind == 'p' && launches[0].steps == 4, "a small batch: one launch of 4 steps");
        CHECK(of(0, 0).size() == 1 && of(0, 0)[0].vx == 2.f && of(0, 1).empty() && of(0, 2).size() == 1 && of(0, 2)[0].member == 2 && of(0, 3).empty(), "rows 0 .. 3");
    }
    // with a recorder on (every = 2) the launch of 5 steps is cut at the frames: 1 step (one was recorded), 2, 2
    CHECK(sfl_batch_record_start(b, 2, 0, B, 1, 1, 4) == SFL_OK && sfl_batch_step_n(b, 1, DT, DX, 3, OMEGA) == SFL_OK, "recorder: %s", sfl_last_error());
    CHECK(sfl_batch_queue_forces_at(b, 4, m2, kCells, kVel, 1) == SFL_OK && sfl_batch_queue_forces_at(b, 6, m0, kCells, kVel, 1) == SFL_OK, "queue");
    applied.clear();
    launches.clear();
    CHECK(sfl_batch_step_n(b, 5, DT, DX, 3, OMEGA) == SFL_OK && pending_is(b, 1, 1), "step_n(5): %s", sfl_last_error());
    if (!large) {
        CHECK(launches.size() == 3 && launches[0].steps == 1 && launches[1].steps == 2 && launches[2].steps == 2 && launches[2].kind == 'p', "cut at the frames");
        CHECK(applied.size() == 1 && applied[0].launch == 2 && applied[0].step == 1 && applied[0].member == 2, "step 4 = step 1 of the third launch");
    } else {
        CHECK(launches.size() == 5 && applied.size() == 1 && applied[0].launch == 4, "step 4 of five launches");
    }
    int frames = 0;
    CHECK(sfl_batch_record_info(b, &frames, nullptr, nullptr) == SFL_OK && frames == 3, "three frames after 6 recorded steps (got %d)", frames);
    CHECK(sfl_batch_record_stop(b) == SFL_OK, "recorder off");
    // forget: the record left at step 1 is never applied
    applied.clear();
    launches.clear();
    CHECK(sfl_batch_forget_forces(b) == SFL_OK && pending_is(b, 0, -1), "forget");
    CHECK(sfl_batch_step_n(b, 3, DT, DX, 3, OMEGA) == SFL_OK && applied.empty() && launches.size() == 3 && launches[1].offsets == nullptr, "nothing applied, per-step launches");
    CHECK(sfl_batch_destroy(b) == SFL_OK, "destroy");
}

int main()
{
    contexts(16, 12);     // the one-workgroup path of a context
    contexts(160, 128);   // tiled kernels, step seams
    linked_ranks();
    batches(false);
    batches(true);
    const long left = fake_hip_live_allocations();
    printf("timeline driver: %d failed checks, %ld allocations left\n", failures, left);
    return failures || left ? 1 : 0;
}
