// views_driver.cpp -- TEST HARNESS (tests/cpp, `make -f views.mk`; tests/test_views.py): the HOST side of the views
// (csrc/views.cpp) and of their hook in the recorder (csrc/batch_frames.cpp), run on a box without a GPU under AddressSanitizer +
// UBSan: the host units of contexts and batches over the runtime that lives on the host (fake_hip.cpp) and kernels that do nothing
// (launch_stubs_ok.cpp).  The launchers of csrc/view_kernels.h and the dye's launch_batch_render are stubs of THIS file that keep
// ONE log in the order of the calls, which is the order of the stream, and fill what they are asked to write with a pattern.
// What is checked: the pointers and strides the launchers are handed for first > 0; the staged palette's bytes and the derived
// constants; exactly the result's bytes reach the host; sfl_batch_record_view before sfl_batch_record_start is SFL_ERR_STATE; its
// reset by record_start and record_stop; a recording that never calls it draws the dye; the staged view does not read the
// caller's memory after the call; refusals with their messages; destroying a context or batch with a staged view leaves no
// allocation.  Exit status 0 and "0 failed checks" = all of it.
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../esp32-fluid-simulation_amd/csrc/batch_state.h"
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
    char kind;   // 'S' scalars, 'T' texels, 'V' a view's images, 'D' the dye's images (launch_batch_render)
    void *out;
    sfl::ViewFields f;
    sfl::ViewParams v;
    int scaling, byteswap;
    const uint32_t *dye;
    std::vector<uint32_t> palette;   // what the device palette held when the launch was made
};
static std::vector<Event> events;

static std::vector<uint32_t> palette_now(const sfl::ViewParams &v)
{
    return v.palette ? std::vector<uint32_t>(v.palette, v.palette + 3 + 3 * v.stops) : std::vector<uint32_t>();
}

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
hipError_t launch_batch_render(hipStream_t, uint16_t *images, const uint32_t *dye, int dim_x, int dim_y, int count, int scaling, bool byteswap)
{
    events.push_back({'D', images, ViewFields{nullptr, nullptr, dim_x, dim_y, count}, ViewParams{}, scaling, byteswap, dye, {}});
    return hipSuccess;
}
// every byte of a result gets 0x50 + what
hipError_t launch_view_scalar(hipStream_t, float *out, const ViewFields &f, int what, float two_dx_inv)
{
    events.push_back({'S', out, f, ViewParams{what, two_dx_inv, 0, 0, 0, nullptr}, 0, 0, nullptr, {}});
    memset(out, 0x50 + what, (size_t)f.count * f.dim_x * f.dim_y * 4);
    return hipSuccess;
}
hipError_t launch_view_texels(hipStream_t, uint32_t *out, const ViewFields &f, const ViewParams &v)
{
    events.push_back({'T', out, f, v, 0, 0, nullptr, palette_now(v)});
    memset(out, 0x50 + v.what, (size_t)f.count * f.dim_x * f.dim_y * 12);
    return hipSuccess;
}
hipError_t launch_view_render(hipStream_t, uint16_t *images, const ViewFields &f, const ViewParams &v, int scaling, bool byteswap)
{
    events.push_back({'V', images, f, v, scaling, byteswap, nullptr, palette_now(v)});
    memset(images, 0x50 + v.what, (size_t)f.count * scaling * (f.dim_x - 1) * scaling * (f.dim_y - 1) * 2);
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

static const uint32_t MAXC = SFL_VIEW_MAX_COLOUR;
static uint32_t g_colours[12] = {0, 0, MAXC, MAXC, MAXC, MAXC, MAXC, 0, 0, 7, 8, 9};
static sfl_view make_view(int what, float dx, float lo, float hi, int stops)
{
    sfl_view v{};
    v.what = what, v.dx = dx, v.lo = lo, v.hi = hi, v.stops = stops;
    v.nan_colour[0] = 11, v.nan_colour[1] = 12, v.nan_colour[2] = 13;
    v.colours = g_colours;
    return v;
}
// nan_colour, then the stops: what the kernels read
static bool palette_is(const std::vector<uint32_t> &got, const sfl_view &v, const uint32_t *colours)
{
    if (got.size() != 3 + 3 * (size_t)v.stops) return false;
    return memcmp(got.data(), v.nan_colour, 12) == 0 && memcmp(got.data() + 3, colours, 12 * (size_t)v.stops) == 0;
}
static bool params_are(const sfl::ViewParams &p, const sfl_view &v, const uint32_t *d_palette)
{
    return p.what == v.what && p.two_dx_inv == 1.0f / (2.0f * v.dx) && p.lo == v.lo && p.r == 1.0f / (v.hi - v.lo) && p.stops == v.stops &&
           p.palette == d_palette;
}

static void refusals_without_objects()
{
    float f[4];
    uint32_t u[12];
    uint16_t h[4];
    sfl_view ok = make_view(SFL_VIEW_VORTICITY, 1.0f, -1.0f, 1.0f, 3), bad = ok;
    CHECK(sfl_view_scalar(nullptr, 4, 1.0f, f, 16) == SFL_ERR_INVALID && says("sfl_view_scalar: unknown view 4"), "what 4: %s", sfl_last_error());
    CHECK(sfl_batch_view_scalar(nullptr, 1, 0.0f, 0, 1, f, 16) == SFL_ERR_INVALID && says("dx must be finite and > 0"), "dx 0: %s", sfl_last_error());
    CHECK(sfl_view_scalar(nullptr, 1, 1.0f, f, 16) == SFL_ERR_INVALID && says("ctx is NULL"), "ctx NULL: %s", sfl_last_error());
    CHECK(sfl_view_texels(nullptr, nullptr, u, 48) == SFL_ERR_INVALID && says("view is NULL"), "view NULL: %s", sfl_last_error());
    bad.stops = 1;
    CHECK(sfl_batch_view_texels(nullptr, &bad, 0, 1, u, 48) == SFL_ERR_INVALID && says("stops must be 2..256 (got 1)"), "stops 1: %s", sfl_last_error());
    bad = ok, bad.colours = nullptr;
    CHECK(sfl_view_render(nullptr, &bad, 1, 1, h, 8) == SFL_ERR_INVALID && says("colours is NULL"), "colours NULL: %s", sfl_last_error());
    bad = ok, bad.hi = bad.lo;
    CHECK(sfl_batch_view_render_members(nullptr, &bad, 0, 1, 1, 1, h, 8) == SFL_ERR_INVALID && says("hi - lo must be finite and > 0"), "hi == lo: %s", sfl_last_error());
    bad = ok, bad.nan_colour[2] = MAXC + 1;
    CHECK(sfl_batch_record_view(nullptr, &bad) == SFL_ERR_INVALID && says("nan_colour channel 2 is 0xFC000001"), "nan_colour: %s", sfl_last_error());
    CHECK(sfl_view_render(nullptr, &ok, 65, 1, h, 8) == SFL_ERR_INVALID && says("scaling must be 1..64 (got 65)"), "scaling 65: %s", sfl_last_error());
    CHECK(sfl_batch_record_view(nullptr, &ok) == SFL_ERR_INVALID && says("batch is NULL") && sfl_batch_record_view(nullptr, nullptr) == SFL_ERR_INVALID, "batch NULL");
    CHECK(events.empty(), "a refused call launches nothing");
}

static void batches(bool large)
{
    const int B = 5, X = 8, Y = 6, CELLS = X * Y;
    sfl_batch *b = nullptr;
    CHECK((large ? sfl_batch_create_large : sfl_batch_create)(&b, 0, X, Y, B) == SFL_OK && b, "create: %s", sfl_last_error());
    if (!b) return;
    events.clear();
    // ---- scalars of members [1, 3): pointers, strides, exactly the result's bytes
    std::vector<uint8_t> host(B * CELLS * 12 + 1, 0);
    CHECK(sfl_batch_view_scalar(b, SFL_VIEW_DIVERGENCE, 0.37f, 1, 2, (float *)host.data(), 2 * CELLS * 4) == SFL_OK && kinds() == "S", "scalar: %s", sfl_last_error());
    if (events.size() == 1) {
        const Event &e = events[0];
        CHECK(e.f.v == b->vel + 2 * 1 * CELLS && e.f.p == b->p + 1 * CELLS && e.f.count == 2 && e.f.dim_x == X && e.f.dim_y == Y, "the fields of member 1 on");
        CHECK(e.out == b->views.d_out && b->views.out_bytes >= 2u * CELLS * 4 && e.v.what == SFL_VIEW_DIVERGENCE && e.v.two_dx_inv == 1.0f / (2.0f * 0.37f), "the launch's result and constants");
        CHECK(host[0] == 0x53 && host[2 * CELLS * 4 - 1] == 0x53 && host[2 * CELLS * 4] == 0, "exactly the scalars' bytes copied out");
    }
    CHECK(sfl_batch_view_scalar(b, 0, 1.0f, 1, 2, (float *)host.data(), 2 * CELLS * 4 - 4) == SFL_ERR_INVALID && says("384 bytes") && says("got 380"), "bytes: %s", sfl_last_error());
    CHECK(sfl_batch_view_scalar(b, 0, 1.0f, 4, 2, (float *)host.data(), 2 * CELLS * 4) == SFL_ERR_INVALID && says("[4, 4 + 2)"), "range: %s", sfl_last_error());
    CHECK(sfl_batch_view_scalar(b, 0, 1.0f, -1, 1, (float *)host.data(), CELLS * 4) == SFL_ERR_INVALID && says("[-1, -1 + 1)"), "range: %s", sfl_last_error());
    CHECK(sfl_batch_view_scalar(b, 0, 1.0f, 1, 2, nullptr, 2 * CELLS * 4) == SFL_ERR_INVALID && says("host is NULL"), "host NULL: %s", sfl_last_error());
    CHECK(sfl_batch_view_scalar(b, 0, 1.0f, 5, 0, nullptr, 0) == SFL_OK && kinds() == "S", "count == 0 does nothing");
    // ---- texels of members [2, 5): the staged palette
    events.clear();
    std::fill(host.begin(), host.end(), 0);
    sfl_view view = make_view(SFL_VIEW_VORTICITY, 0.5f, -2.0f, 6.0f, 4);
    CHECK(sfl_batch_view_texels(b, &view, 2, 3, (uint32_t *)host.data(), 3 * CELLS * 12) == SFL_OK && kinds() == "T", "texels: %s", sfl_last_error());
    if (events.size() == 1) {
        const Event &e = events[0];
        CHECK(e.f.v == b->vel + 2 * 2 * CELLS && e.f.p == b->p + 2 * CELLS && e.f.count == 3, "the fields of member 2 on");
        CHECK(params_are(e.v, view, b->views.d_palette) && palette_is(e.palette, view, g_colours), "the derived constants and the staged palette");
        CHECK(e.out == b->views.d_out && host[0] == 0x51 && host[3 * CELLS * 12 - 1] == 0x51 && host[3 * CELLS * 12] == 0, "exactly the texels' bytes");
    }
    CHECK(sfl_batch_view_texels(b, &view, 2, 3, (uint32_t *)host.data(), 3 * CELLS * 4) == SFL_ERR_INVALID && says("1728 bytes"), "bytes: %s", sfl_last_error());
    // ---- images of members [1, 4) at scaling 2
    events.clear();
    const size_t one = 2 * (X - 1) * 2 * (Y - 1) * 2;
    std::vector<uint8_t> img(B * one + 1, 0);
    view = make_view(SFL_VIEW_PRESSURE, 1.0f, 0.0f, 1.0f, 2);
    CHECK(sfl_batch_view_render_members(b, &view, 1, 3, 2, 0, (uint16_t *)img.data(), 3 * one) == SFL_OK && kinds() == "V", "render: %s", sfl_last_error());
    if (events.size() == 1) {
        const Event &e = events[0];
        CHECK(e.f.v == b->vel + 2 * CELLS && e.f.p == b->p + CELLS && e.f.count == 3 && e.scaling == 2 && e.byteswap == 0 && e.out == b->views.d_out, "the launch");
        CHECK(params_are(e.v, view, b->views.d_palette) && palette_is(e.palette, view, g_colours) && img[3 * one - 1] == 0x52 && img[3 * one] == 0, "palette and bytes");
    }
    CHECK(sfl_batch_view_render_members(b, &view, 1, 3, 2, 0, (uint16_t *)img.data(), 3 * one - 2) == SFL_ERR_INVALID && says("3 images of 14 x 10 uint16"), "bytes: %s", sfl_last_error());
    CHECK(sfl_batch_view_render_members(b, &view, 1, 3, 2, 0, nullptr, 3 * one) == SFL_ERR_INVALID && says("host_images is NULL"), "NULL: %s", sfl_last_error());
    CHECK(sfl_batch_view_render_members(b, &view, 0, 0, 2, 0, nullptr, 0) == SFL_OK && kinds() == "V", "count == 0 does nothing");
    // ---- the recorder
    events.clear();
    view = make_view(SFL_VIEW_VORTICITY, 1.0f, -1.0f, 1.0f, 3);
    CHECK(sfl_batch_record_view(b, &view) == SFL_ERR_STATE && says("not recording") && sfl_batch_record_view(b, nullptr) == SFL_ERR_STATE, "before record_start: %s", sfl_last_error());
    CHECK(b->d_rec_palette == nullptr && b->record_view_frame == nullptr && events.empty(), "a refused record_view stages nothing");
    CHECK(sfl_batch_record_start(b, 1, 1, 3, 2, 1, 8) == SFL_OK && sfl_batch_step_n(b, 2, DT, DX, 3, OMEGA) == SFL_OK && kinds() == "DD", "a recording that never calls it: %s", kinds().c_str());
    CHECK(events[0].dye == b->col_tmp + 3 * CELLS || events[0].dye == b->col + 3 * CELLS, "the dye of member 1 on");
    uint32_t mine[9];
    memcpy(mine, g_colours, sizeof mine);
    sfl_view own = view;
    own.colours = mine;
    CHECK(sfl_batch_record_view(b, &own) == SFL_OK && b->rec.view_on && b->d_rec_palette && b->record_view_frame, "record_view: %s", sfl_last_error());
    memset(mine, 0xEE, sizeof mine);   // the caller's memory is not read after the call
    own.lo = 55.0f;
    events.clear();
    CHECK(sfl_batch_step_n(b, 2, DT, DX, 3, OMEGA) == SFL_OK && kinds() == "VV", "frames by the view: %s", kinds().c_str());
    if (events.size() == 2) {
        const size_t frame = 3 * one / 2;   // pixels of one frame
        CHECK(events[0].out == b->d_frames + 2 * frame && events[1].out == b->d_frames + 3 * frame, "frames 2 and 3 of the recording");
        CHECK(events[1].f.v == b->vel + 2 * CELLS && events[1].f.p == b->p + CELLS && events[1].f.count == 3 && events[1].scaling == 2 && events[1].byteswap == 1,
              "the velocity the step left, members [1, 4)");
        CHECK(params_are(events[1].v, view, b->d_rec_palette) && palette_is(events[1].palette, view, g_colours), "the view as it was at the call");
    }
    int frames = -1;
    CHECK(sfl_batch_record_info(b, &frames, nullptr, nullptr) == SFL_OK && frames == 4, "frames keep their count");
    // a view call between the frames has its own palette buffer
    sfl_view other = make_view(SFL_VIEW_SPEED, 1.0f, 0.0f, 9.0f, 2);
    other.colours = g_colours + 3;
    CHECK(sfl_batch_view_texels(b, &other, 0, 1, (uint32_t *)host.data(), CELLS * 12) == SFL_OK && b->views.d_palette != b->d_rec_palette, "two buffers");
    events.clear();
    CHECK(sfl_batch_step_n(b, 1, DT, DX, 3, OMEGA) == SFL_OK && kinds() == "V" && palette_is(events[0].palette, view, g_colours), "the recorder's palette is untouched");
    events.clear();
    CHECK(sfl_batch_record_view(b, nullptr) == SFL_OK && !b->rec.view_on && sfl_batch_step_n(b, 1, DT, DX, 3, OMEGA) == SFL_OK && kinds() == "D", "NULL: the dye again");
    // reset by record_start and record_stop
    CHECK(sfl_batch_record_view(b, &view) == SFL_OK && sfl_batch_record_start(b, 1, 0, B, 1, 1, 2) == SFL_OK && !b->rec.view_on, "record_start resets to the dye");
    events.clear();
    CHECK(sfl_batch_step_n(b, 1, DT, DX, 3, OMEGA) == SFL_OK && kinds() == "D", "... and draws it: %s", kinds().c_str());
    CHECK(sfl_batch_record_view(b, &view) == SFL_OK && sfl_batch_record_stop(b) == SFL_OK && !b->rec.view_on, "record_stop resets");
    CHECK(sfl_batch_record_view(b, &view) == SFL_ERR_STATE && sfl_batch_step_n(b, 1, DT, DX, 3, OMEGA) == SFL_OK, "stopped: SFL_ERR_STATE again");
    // ---- destroy with a staged view and a live recording
    CHECK(sfl_batch_record_start(b, 1, 0, B, 1, 1, 2) == SFL_OK && sfl_batch_record_view(b, &view) == SFL_OK && sfl_batch_step_n(b, 1, DT, DX, 3, OMEGA) == SFL_OK, "a live view");
    CHECK(sfl_batch_destroy(b) == SFL_OK, "destroy");
    events.clear();
}

static void contexts()
{
    sfl_context *c = nullptr, *slab = nullptr, *wide = nullptr;
    CHECK(sfl_create(&c, 0, 160, 128) == SFL_OK && sfl_create_slab(&slab, 0, 160, 128, 0, 2) == SFL_OK && sfl_create(&wide, 0, 1025, 1025) == SFL_OK,
          "create: %s", sfl_last_error());
    if (!c || !slab || !wide) return;
    const size_t CELLS = 160 * 128;
    std::vector<uint8_t> host(CELLS * 12 + 1, 0);
    sfl_view view = make_view(SFL_VIEW_DIVERGENCE, 0.25f, -1.0f, 1.0f, 3);
    CHECK(sfl_view_scalar(slab, 0, 1.0f, (float *)host.data(), 4) == SFL_ERR_STATE && says("whole-domain context (slab 0/2)"), "a slab: %s", sfl_last_error());
    CHECK(sfl_view_texels(slab, &view, (uint32_t *)host.data(), 4) == SFL_ERR_STATE && sfl_view_render(slab, &view, 1, 1, (uint16_t *)host.data(), 4) == SFL_ERR_STATE, "a slab");
    events.clear();
    CHECK(sfl_step_n(c, 3, DT, DX, 3, OMEGA) == SFL_OK && sfl_view_scalar(c, SFL_VIEW_PRESSURE, 1.0f, (float *)host.data(), CELLS * 4) == SFL_OK && kinds() == "S",
          "scalar behind step_n: %s (%s)", kinds().c_str(), sfl_last_error());
    if (events.size() == 1)
        CHECK(events[0].f.v == c->vel && events[0].f.p == c->p && events[0].f.count == 1 && events[0].f.dim_x == 160 && events[0].f.dim_y == 128 && events[0].out == c->views.d_out &&
                  host[CELLS * 4 - 1] == 0x52 && host[CELLS * 4] == 0, "the context's own fields, a batch of one");
    CHECK(sfl_view_scalar(c, 0, 1.0f, (float *)host.data(), CELLS * 4 + 4) == SFL_ERR_INVALID && says("81920 bytes") && sfl_view_scalar(c, 0, 1.0f, nullptr, CELLS * 4) == SFL_ERR_INVALID,
          "bytes, NULL: %s", sfl_last_error());
    events.clear();
    CHECK(sfl_view_texels(c, &view, (uint32_t *)host.data(), CELLS * 12) == SFL_OK && kinds() == "T" && params_are(events[0].v, view, c->views.d_palette) &&
              palette_is(events[0].palette, view, g_colours) && host[CELLS * 12 - 1] == 0x53 && host[CELLS * 12] == 0, "texels: %s", sfl_last_error());
    events.clear();
    std::vector<uint8_t> img(159 * 127 * 2 + 1, 0);
    CHECK(sfl_view_render(c, &view, 1, 1, (uint16_t *)img.data(), 159 * 127 * 2) == SFL_OK && kinds() == "V" && events[0].f.v == c->vel && events[0].scaling == 1 &&
              events[0].byteswap == 1 && img[159 * 127 * 2 - 1] == 0x53 && img[159 * 127 * 2] == 0, "render: %s", sfl_last_error());
    CHECK(sfl_view_render(c, &view, 1, 1, (uint16_t *)img.data(), 159 * 127 * 2 + 2) == SFL_ERR_INVALID && says("1 images of 159 x 127 uint16"), "bytes: %s", sfl_last_error());
    // an image whose pixels do not fit the kernel's 32-bit offsets is refused, not overflowed: 1024^2 blocks at scaling 64 = 2^32 pixels
    events.clear();
    CHECK(sfl_view_render(wide, &view, 64, 1, (uint16_t *)img.data(), (size_t)65536 * 65536 * 2) == SFL_ERR_INVALID && says("exceeds the 2^31 - 1 pixels") && events.empty(),
          "too many pixels: %s", sfl_last_error());
    for (sfl_context *x : {c, slab, wide}) CHECK(sfl_destroy(x) == SFL_OK, "destroy");
    events.clear();
}

int main()
{
    refusals_without_objects();
    contexts();
    batches(false);
    batches(true);
    const long left = fake_hip_live_allocations();
    printf("views driver: %d failed checks, %ld allocations left\n", failures, left);
    return failures || left ? 1 : 0;
}
