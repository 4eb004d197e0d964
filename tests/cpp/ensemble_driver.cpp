// ensemble_driver.cpp -- TEST HARNESS (tests/cpp, `make -f ensemble.mk`; tests/test_ensemble.py): the HOST side of sfl_distance,
// sfl_batch_distance and sfl_batch_envelope* (csrc/ensemble.cpp), run on a box without a GPU under AddressSanitizer + UBSan:
// the host units of contexts and batches over the runtime that lives on the host (fake_hip.cpp) and kernels that do nothing
// (launch_stubs_ok.cpp).  The launchers of csrc/ensemble_kernels.h and the draw launcher are stubs of THIS file that keep a log
// of what they are handed; "device" memory is host memory here, so the stubs also leave marks in the records and fields that
// the calls must copy out.  What is checked: every refusal, in the header's order and with its own message, launches nothing
// and leaves sfl_batch_envelope_info and the validity of sfl_batch_residual as they were; the base pointers and member strides
// of both sides for ref == NULL, ref == b, another batch (of the other kind), a fixed ref_member and the pairwise form; the
// records and `what` copied out; the range sfl_batch_envelope_info reports; SFL_ERR_STATE of download / render before the
// first envelope; and that destroy frees everything.  Exit status 0 and "0 failed checks" = every call did what the header says.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../esp32-fluid-simulation_amd/csrc/batch_state.h"
#include "../../esp32-fluid-simulation_amd/csrc/ensemble_kernels.h"
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

// ---- the logs of the launchers ---------------------------------------------------------------------------------------------
struct DistanceLaunch {
    sfl::DistanceRecord *out;
    int what;
    sfl::DistanceSide a, b;
    size_t cells;
    int members;
};
struct EnvelopeLaunch {
    uint32_t *fields, *partials;
    const uint32_t *dye;
    size_t member_words;
    int count;
};
struct RenderLaunch {
    uint16_t *images;
    const uint32_t *colour;
    int count, scaling;
};
static std::vector<DistanceLaunch> distances;
static std::vector<EnvelopeLaunch> envelopes;
static std::vector<RenderLaunch> renders;

namespace sfl {
bool small_grid_fits(int dim_x, int dim_y)   // (the real rule of small_grid.hip; launch_stubs_ok.cpp's answer is "no")
{
    return dim_x >= 2 && dim_y >= 2 && (long long)dim_x * dim_y <= kSmallGridMaxCells &&
           (long long)dim_y * ((dim_x + 1) / 2) <= kSmallGridMaxCells / 2;
}
hipError_t launch_batch_step(hipStream_t, const BatchStep &, int) { return hipSuccess; }
hipError_t launch_batch_step_each(hipStream_t, const BatchStep &, int, const BatchMember *, float *) { return hipSuccess; }
hipError_t launch_batch_step_until(hipStream_t, const BatchStep &, int, const BatchMember *, const BatchStop *, float *, int *, bool) { return hipSuccess; }
hipError_t launch_batch_large_step(hipStream_t, const BatchStep &, int) { return hipSuccess; }
hipError_t launch_batch_large_step_each(hipStream_t, const BatchStep &, int, const BatchMember *, float *) { return hipSuccess; }
hipError_t launch_batch_large_step_until(hipStream_t, const BatchStep &, int, const BatchMember *, const BatchStop *, float *, int *, bool) { return hipSuccess; }
hipError_t launch_batch_play(hipStream_t, const BatchPlay &, int, const BatchMember *, float *) { return hipSuccess; }
hipError_t launch_batch_solve(hipStream_t, float *, const float *, int, int, int, int, SorParams) { return hipSuccess; }
hipError_t launch_batch_solve_each(hipStream_t, float *, const float *, int, int, int, const BatchMember *, float *) { return hipSuccess; }
hipError_t launch_batch_solve_until(hipStream_t, float *, const float *, int, int, int, const BatchMember *, const BatchStop *, float *, int *) { return hipSuccess; }
hipError_t launch_batch_large_solve(hipStream_t, float *, const float *, int, int, int, int, SorParams) { return hipSuccess; }
hipError_t launch_batch_large_solve_each(hipStream_t, float *, const float *, int, int, int, const BatchMember *, float *) { return hipSuccess; }
hipError_t launch_batch_large_solve_until(hipStream_t, float *, const float *, int, int, int, const BatchMember *, const BatchStop *, float *, int *) { return hipSuccess; }
hipError_t launch_flow_stats(hipStream_t, FlowStatsRecord *, int, const float *, const uint32_t *, int, int, int, float, const float *) { return hipSuccess; }
hipError_t launch_batch_render(hipStream_t, uint16_t *images, const uint32_t *colour, int dim_x, int dim_y, int count, int scaling, bool)
{
    renders.push_back({images, colour, count, scaling});
    const size_t pixels = (size_t)count * scaling * (dim_x - 1) * scaling * (dim_y - 1);
    for (size_t k = 0; k < pixels; ++k) images[k] = (uint16_t)colour[0];   // (the first word of the field drawn)
    return hipSuccess;
}
// record k gets the marks 100 + k, 200 + k, 300 + k in its three counts: the call must copy them out, and fill in `what`
hipError_t launch_field_distance(hipStream_t, DistanceRecord *out, int what, const DistanceSide &a, const DistanceSide &b, size_t cells, int members)
{
    distances.push_back({out, what, a, b, cells, members});
    memset(out, 0, sizeof(DistanceRecord) * (size_t)members);
    for (int k = 0; k < members; ++k) {
        out[k].velocity_cells_differ = 100u + k;
        out[k].dye_cells_differ = 200u + k;
        out[k].pressure_cells_differ = 300u + k;
    }
    return hipSuccess;
}
// every word of field `which` gets 1000 * (which + 1) + count; the partials are written from end to end
hipError_t launch_batch_envelope(hipStream_t, uint32_t *fields, uint32_t *partials, const uint32_t *dye, size_t member_words, int count)
{
    envelopes.push_back({fields, partials, dye, member_words, count});
    for (int which = 0; which < 4; ++which)
        for (size_t w = 0; w < member_words; ++w) fields[which * member_words + w] = 1000u * (which + 1) + count;
    memset(partials, 0x5a, sizeof(uint32_t) * envelope_partial_words(count, member_words));
    return hipSuccess;
}
}  // namespace sfl

static const float DT = 0.03f, DX = 1.0f, OMEGA = 1.9f;

static bool info_is(sfl_batch *b, int first, int count)
{
    int f = -7, c = -7;
    return sfl_batch_envelope_info(b, &f, &c) == SFL_OK && f == first && c == count;
}
static bool residual_valid(sfl_batch *b)
{
    float r[1];
    return sfl_batch_residual(b, 0, 1, r, sizeof r) == SFL_OK;
}
static bool says(const char *word) { return strstr(sfl_last_error(), word) != nullptr; }
static size_t launches() { return distances.size() + envelopes.size() + renders.size(); }

// the checks that need no handle: each answers with its own message, in the header's order
static void refusals_without_handles()
{
    struct sfl_field_distance rec[2];
    CHECK(sfl_distance(nullptr, nullptr, 0, nullptr) == SFL_ERR_INVALID && says("what must be"), "what 0: %s", sfl_last_error());
    CHECK(sfl_distance(nullptr, nullptr, 8, rec) == SFL_ERR_INVALID && says("got 8"), "what 8: %s", sfl_last_error());
    CHECK(sfl_distance(nullptr, nullptr, 7, rec) == SFL_ERR_INVALID && says("NULL"), "NULL contexts: %s", sfl_last_error());
    CHECK(sfl_batch_distance(nullptr, 0, nullptr, 0, 0, 2, rec, 1) == SFL_ERR_INVALID && says("what must be"), "what before bytes: %s", sfl_last_error());
    CHECK(sfl_batch_distance(nullptr, 16, nullptr, 0, 0, 2, rec, sizeof rec) == SFL_ERR_INVALID && says("got 16"), "what 16: %s", sfl_last_error());
    CHECK(sfl_batch_distance(nullptr, 3, nullptr, 0, 0, 2, rec, 127) == SFL_ERR_INVALID && says("128 bytes"), "bytes before NULL: %s", sfl_last_error());
    CHECK(sfl_batch_distance(nullptr, 3, nullptr, 0, 0, -1, rec, 0) == SFL_ERR_INVALID && says("bytes"), "count < 0: %s", sfl_last_error());
    CHECK(sfl_batch_distance(nullptr, 3, nullptr, 0, 0, 2, rec, sizeof rec) == SFL_ERR_INVALID && says("NULL"), "NULL batch: %s", sfl_last_error());
    uint32_t word[1];
    uint16_t pixel[1];
    CHECK(sfl_batch_envelope(nullptr, 0, 1) == SFL_ERR_INVALID && sfl_batch_envelope_info(nullptr, nullptr, nullptr) == SFL_ERR_INVALID, "NULL batch");
    CHECK(sfl_batch_envelope_download(nullptr, 4, word, 4) == SFL_ERR_INVALID && says("which must be"), "which 4: %s", sfl_last_error());
    CHECK(sfl_batch_envelope_download(nullptr, -1, word, 4) == SFL_ERR_INVALID && says("got -1"), "which -1: %s", sfl_last_error());
    CHECK(sfl_batch_envelope_download(nullptr, 0, word, 4) == SFL_ERR_INVALID && says("NULL"), "NULL batch: %s", sfl_last_error());
    CHECK(sfl_batch_envelope_render(nullptr, 4, 0, 1, pixel, 2) == SFL_ERR_INVALID && says("which must be"), "which before scaling: %s", sfl_last_error());
    CHECK(sfl_batch_envelope_render(nullptr, 3, 0, 1, pixel, 2) == SFL_ERR_INVALID && says("scaling must be 1..64"), "scaling 0: %s", sfl_last_error());
    CHECK(sfl_batch_envelope_render(nullptr, 3, 65, 1, pixel, 2) == SFL_ERR_INVALID && says("got 65"), "scaling 65: %s", sfl_last_error());
    CHECK(sfl_batch_envelope_render(nullptr, 3, 1, 1, pixel, 2) == SFL_ERR_INVALID && says("NULL"), "NULL batch: %s", sfl_last_error());
    CHECK(launches() == 0, "a refused call launches nothing");
}

static bool side_is(const sfl::DistanceSide &s, const sfl_batch *b, int member, size_t stride)
{
    const size_t at = (size_t)member * b->cells;
    return s.v == b->vel + 2 * at && s.dye == b->col + 3 * at && s.p == b->p + at && s.member_cells == stride;
}

static void batches(bool large)
{
    const int B = 5, X = 8, Y = 6;
    sfl_batch *b = nullptr, *twin = nullptr, *other = nullptr, *few = nullptr;
    CHECK((large ? sfl_batch_create_large : sfl_batch_create)(&b, 0, X, Y, B) == SFL_OK && b, "create: %s", sfl_last_error());
    CHECK((large ? sfl_batch_create : sfl_batch_create_large)(&twin, 0, X, Y, B) == SFL_OK && twin, "the twin of the other kind: %s", sfl_last_error());
    CHECK(sfl_batch_create(&other, 0, X, Y + 1, B) == SFL_OK && sfl_batch_create(&few, 0, X, Y, 3) == SFL_OK, "create: %s", sfl_last_error());
    if (!b || !twin || !other || !few) return;
    const size_t cells = (size_t)X * Y;
    sfl_member_params prm[B];
    for (int m = 0; m < B; ++m) prm[m] = {DT, DX, OMEGA, 3 + m};
    CHECK(sfl_batch_step_n_each(b, 1, prm) == SFL_OK && residual_valid(b), "a valid residual report: %s", sfl_last_error());
    CHECK(info_is(b, 0, 0), "a fresh batch holds no envelope");
    struct sfl_field_distance rec[B];
    std::vector<uint32_t> field(3 * cells);
    std::vector<uint16_t> image((size_t)2 * (X - 1) * 2 * (Y - 1));
    distances.clear(), envelopes.clear(), renders.clear();

    // ---- refusals: nothing launched, envelope_info and the residual's validity as they were
    CHECK(sfl_batch_envelope_download(b, 0, field.data(), field.size() * 4) == SFL_ERR_STATE && says("sfl_batch_envelope"), "download before an envelope: %s", sfl_last_error());
    CHECK(sfl_batch_envelope_render(b, 0, 2, 1, image.data(), image.size() * 2) == SFL_ERR_STATE, "render before an envelope: %s", sfl_last_error());
    CHECK(sfl_batch_envelope_download(b, 0, field.data(), field.size() * 4 - 4) == SFL_ERR_INVALID && says("576 bytes"), "download bytes: %s", sfl_last_error());
    CHECK(sfl_batch_envelope_download(b, 0, nullptr, field.size() * 4) == SFL_ERR_INVALID && says("NULL"), "download NULL: %s", sfl_last_error());
    CHECK(sfl_batch_envelope_render(b, 0, 2, 1, image.data(), image.size() * 2 + 2) == SFL_ERR_INVALID && says("280 bytes"), "render bytes: %s", sfl_last_error());
    CHECK(sfl_batch_envelope_render(b, 0, 2, 1, nullptr, image.size() * 2) == SFL_ERR_INVALID && says("NULL"), "render NULL: %s", sfl_last_error());
    CHECK(sfl_batch_envelope(b, 0, 0) == SFL_ERR_INVALID && says("count must be >= 1"), "count 0: %s", sfl_last_error());
    CHECK(sfl_batch_envelope(b, -1, 2) == SFL_ERR_INVALID && sfl_batch_envelope(b, 3, 3) == SFL_ERR_INVALID && says("not inside"), "range: %s", sfl_last_error());
    CHECK(sfl_batch_distance(b, 7, nullptr, 0, 0, B, nullptr, sizeof rec) == SFL_ERR_INVALID && says("NULL"), "host NULL: %s", sfl_last_error());
    CHECK(sfl_batch_distance(b, 7, nullptr, 0, 2, 4, rec, 4 * 64) == SFL_ERR_INVALID && says("not inside the batch"), "range: %s", sfl_last_error());
    CHECK(sfl_batch_distance(b, 7, nullptr, 0, -1, 1, rec, 64) == SFL_ERR_INVALID && says("not inside the batch"), "first < 0: %s", sfl_last_error());
    CHECK(sfl_batch_distance(b, 7, nullptr, B, 0, 1, rec, 64) == SFL_ERR_INVALID && says("ref_member 5"), "ref_member == B: %s", sfl_last_error());
    CHECK(sfl_batch_distance(b, 7, nullptr, -2, 0, 1, rec, 64) == SFL_ERR_INVALID && says("ref_member -2"), "ref_member -2: %s", sfl_last_error());
    CHECK(sfl_batch_distance(b, 7, few, 3, 0, 1, rec, 64) == SFL_ERR_INVALID && says("[0, 3)"), "ref_member outside ref: %s", sfl_last_error());
    CHECK(sfl_batch_distance(b, 7, few, -1, 2, 2, rec, 128) == SFL_ERR_INVALID && says("pairwise"), "a pairwise range outside ref: %s", sfl_last_error());
    CHECK(sfl_batch_distance(b, 7, other, 0, 0, B, rec, sizeof rec) == SFL_ERR_INVALID && says("shapes must be the same"), "shape: %s", sfl_last_error());
    CHECK(sfl_batch_distance(b, 7, other, B, 0, B, rec, sizeof rec) == SFL_ERR_INVALID && says("ref_member"), "the range comes before the shape: %s", sfl_last_error());
    CHECK(launches() == 0 && info_is(b, 0, 0) && residual_valid(b), "the refused calls launched nothing and changed nothing");
    CHECK(b->d_dist == nullptr && b->d_env == nullptr, "... and allocated nothing");
    CHECK(sfl_batch_distance(b, 7, nullptr, 0, 2, 0, rec, 0) == SFL_OK && sfl_batch_distance(b, 7, nullptr, 0, B, 0, nullptr, 0) == SFL_ERR_INVALID && launches() == 0,
          "count 0 does nothing");

    // ---- the two sides handed to the launcher
    memset(rec, 0xff, sizeof rec);
    CHECK(sfl_batch_distance(b, 7, nullptr, 2, 0, B, rec, sizeof rec) == SFL_OK && distances.size() == 1, "ref NULL: %s", sfl_last_error());
    if (distances.size() == 1) {
        const DistanceLaunch &l = distances[0];
        CHECK(l.what == 7 && l.cells == cells && l.members == B && l.out == reinterpret_cast<sfl::DistanceRecord *>(b->d_dist), "what, cells, members, records");
        CHECK(side_is(l.a, b, 0, cells) && side_is(l.b, b, 2, 0), "every member of b against member 2 of b: stride 0");
    }
    for (int k = 0; k < B; ++k)
        CHECK(rec[k].what == 7u && rec[k].velocity_cells_differ == 100u + k && rec[k].dye_cells_differ == 200u + k && rec[k].pressure_cells_differ == 300u + k &&
                  rec[k].max_abs_dvx == 0.0f && rec[k].sum_abs_ddye[2] == 0, "record %d copied out, `what` filled in", k);
    CHECK(sfl_batch_distance(b, 2, b, 4, 1, 3, rec, 3 * 64) == SFL_OK && distances.size() == 2, "ref == b: %s", sfl_last_error());
    if (distances.size() == 2) {
        const DistanceLaunch &l = distances[1];
        CHECK(l.what == 2 && l.members == 3 && side_is(l.a, b, 1, cells) && side_is(l.b, b, 4, 0), "members [1, 4) of b against member 4 of b");
        CHECK(rec[0].what == 2u && rec[2].dye_cells_differ == 202u && rec[3].what == 7u, "three records written, the fourth left");
    }
    CHECK(sfl_batch_distance(b, 5, twin, 0, 3, 2, rec, 2 * 64) == SFL_OK && distances.size() == 3, "another batch, fixed member: %s", sfl_last_error());
    if (distances.size() == 3) CHECK(side_is(distances[2].a, b, 3, cells) && side_is(distances[2].b, twin, 0, 0), "members [3, 5) of b against member 0 of the twin");
    CHECK(sfl_batch_distance(b, 7, twin, -1, 1, 4, rec, 4 * 64) == SFL_OK && distances.size() == 4, "pairwise: %s", sfl_last_error());
    if (distances.size() == 4) CHECK(side_is(distances[3].a, b, 1, cells) && side_is(distances[3].b, twin, 1, cells), "member 1 + k of b against member 1 + k of the twin");
    CHECK(sfl_batch_distance(b, 1, few, -1, 0, 3, rec, 3 * 64) == SFL_OK && distances.size() == 5, "pairwise against a shorter batch: %s", sfl_last_error());
    CHECK(sfl_batch_distance(b, 4, nullptr, -1, 0, B, rec, sizeof rec) == SFL_OK && distances.size() == 6, "pairwise against itself: %s", sfl_last_error());
    if (distances.size() == 6) CHECK(side_is(distances[5].a, b, 0, cells) && side_is(distances[5].b, b, 0, cells), "b against b");
    CHECK(residual_valid(b) && residual_valid(b) && info_is(b, 0, 0) && envelopes.empty(), "distances read only");

    // ---- the envelope: the range held, the fields copied out, the draw launch on the field asked for
    CHECK(sfl_batch_envelope(b, 1, 3) == SFL_OK && envelopes.size() == 1 && info_is(b, 1, 3), "envelope of [1, 4): %s", sfl_last_error());
    if (envelopes.size() == 1) {
        const EnvelopeLaunch &l = envelopes[0];
        CHECK(l.dye == b->col + 3 * cells && l.member_words == 3 * cells && l.count == 3 && l.fields == b->d_env && l.partials == b->d_env + 12 * cells,
              "the dye of member 1, 3 members, the fields and the partials behind them");
    }
    CHECK(sfl_batch_envelope(b, 4, 2) == SFL_ERR_INVALID && sfl_batch_envelope(b, 0, -1) == SFL_ERR_INVALID && info_is(b, 1, 3) && envelopes.size() == 1,
          "a refused envelope leaves the snapshot");
    CHECK(sfl_batch_envelope_info(b, nullptr, nullptr) == SFL_OK, "both out pointers may be NULL");
    CHECK(sfl_batch_envelope_download(b, SFL_ENV_MAX, field.data(), field.size() * 4) == SFL_OK && field[0] == 3003u && field[3 * cells - 1] == 3003u,
          "the maximum copied out: %s", sfl_last_error());
    CHECK(sfl_batch_envelope_download(b, 7, field.data(), field.size() * 4) == SFL_ERR_INVALID && info_is(b, 1, 3), "which 7");
    CHECK(sfl_batch_envelope_render(b, SFL_ENV_SPREAD, 2, 1, image.data(), image.size() * 2) == SFL_OK && renders.size() == 1, "render: %s", sfl_last_error());
    if (renders.size() == 1)
        CHECK(renders[0].colour == b->d_env + 3 * 3 * cells && renders[0].count == 1 && renders[0].scaling == 2 && image[0] == 4003u && image.back() == 4003u,
              "one image of the spread");
    CHECK(sfl_batch_envelope(b, 0, B) == SFL_OK && info_is(b, 0, B) && envelopes.size() == 2 && envelopes[1].fields == envelopes[0].fields, "the next envelope replaces it");
    CHECK(sfl_batch_step_n_each(b, 2, prm) == SFL_OK && info_is(b, 0, B) && residual_valid(b), "steps leave the snapshot's range: %s", sfl_last_error());
    CHECK(sfl_batch_envelope_download(b, SFL_ENV_MEAN, field.data(), field.size() * 4) == SFL_OK && field[5] == 1005u, "the mean of 5 members");
    CHECK(residual_valid(b), "the envelope calls read only");
    for (sfl_batch *x : {b, twin, other, few}) CHECK(sfl_batch_destroy(x) == SFL_OK, "destroy");
}

static void contexts()
{
    sfl_context *a = nullptr, *b = nullptr, *wide = nullptr, *slab = nullptr;
    CHECK(sfl_create(&a, 0, 16, 12) == SFL_OK && sfl_create(&b, 0, 16, 12) == SFL_OK && sfl_create(&wide, 0, 17, 12) == SFL_OK &&
              sfl_create_slab(&slab, 0, 16, 12, 0, 2) == SFL_OK, "create: %s", sfl_last_error());
    if (!a || !b || !wide || !slab) return;
    struct sfl_field_distance rec;
    distances.clear();
    CHECK(sfl_distance(a, b, 0, &rec) == SFL_ERR_INVALID && sfl_distance(a, b, 9, &rec) == SFL_ERR_INVALID && says("what must be"), "what: %s", sfl_last_error());
    CHECK(sfl_distance(a, nullptr, 7, &rec) == SFL_ERR_INVALID && sfl_distance(nullptr, b, 7, &rec) == SFL_ERR_INVALID && sfl_distance(a, b, 7, nullptr) == SFL_ERR_INVALID, "NULL");
    CHECK(sfl_distance(a, slab, 7, &rec) == SFL_ERR_STATE && says("whole-domain") && sfl_distance(slab, slab, 1, &rec) == SFL_ERR_STATE, "a slab: %s", sfl_last_error());
    CHECK(sfl_distance(a, wide, 7, &rec) == SFL_ERR_INVALID && says("shapes must be the same"), "shape: %s", sfl_last_error());
    CHECK(distances.empty() && a->d_dist == nullptr, "the refused calls launched and allocated nothing");
    memset(&rec, 0xff, sizeof rec);
    CHECK(sfl_distance(a, b, 7, &rec) == SFL_OK && distances.size() == 1, "distance: %s", sfl_last_error());
    if (distances.size() == 1) {
        const DistanceLaunch &l = distances[0];
        CHECK(l.what == 7 && l.cells == 16u * 12u && l.members == 1 && l.out == reinterpret_cast<sfl::DistanceRecord *>(a->d_dist), "one member of 192 cells");
        CHECK(l.a.v == a->vel && l.a.dye == a->col && l.a.p == a->p && l.b.v == b->vel && l.b.dye == b->col && l.b.p == b->p && a->vel && b->col && b->p, "the fields of a and b");
    }
    CHECK(rec.what == 7u && rec.velocity_cells_differ == 100u && rec.pressure_cells_differ == 300u && b->d_dist == nullptr, "the record copied out; a's records only");
    const struct sfl_field_distance *kept = a->d_dist;
    CHECK(sfl_distance(a, a, 2, &rec) == SFL_OK && distances.size() == 2 && distances[1].a.dye == a->col && distances[1].b.dye == a->col && rec.what == 2u, "a == b: %s", sfl_last_error());
    CHECK(a->d_dist == kept, "nothing is allocated per call");
    for (sfl_context *c : {a, b, wide, slab}) CHECK(sfl_destroy(c) == SFL_OK, "destroy");
}

int main()
{
    refusals_without_handles();
    batches(false);
    batches(true);
    contexts();
    const long left = fake_hip_live_allocations();
    printf("ensemble driver: %d failed checks, %ld allocations left\n", failures, left);
    return failures || left ? 1 : 0;
}
