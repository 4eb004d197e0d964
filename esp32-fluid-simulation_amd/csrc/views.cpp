// views.cpp -- the flow itself as pictures (include/sfl.h "VIEWS"): sfl_view_* of a whole-domain context, sfl_batch_view_*
// of a batch of either kind, and sfl_batch_record_view, which says what the recorder's frames show.  Host C++ only; the
// kernels are field_view.hip (view_kernels.h).
//
// One body serves contexts and batches: a Holder names the stream, the shape, the fields of the first member asked for and
// the member count (1 for a context).  Every refusal is made before any GPU work.  The units of the step calls and of
// the recorder are linked without this one by the host test harnesses, so they do not call into it: what a view keeps on
// the device is plain data on the two structs (context.h ViewScratch, batch_state.h), freed by their destroy paths, and
// the recorder reaches the view's render through the batch's `record_view_frame` pointer, set here.
#include <cmath>
#include <vector>

#include "batch_state.h"
#include "view_kernels.h"

using namespace sfl::host;

static_assert(sizeof(struct sfl_view) == 40 && offsetof(struct sfl_view, dx) == 4 && offsetof(struct sfl_view, lo) == 8 &&
                  offsetof(struct sfl_view, hi) == 12 && offsetof(struct sfl_view, stops) == 16 &&
                  offsetof(struct sfl_view, nan_colour) == 20 && offsetof(struct sfl_view, colours) == 32,
              "sfl_view: 40 bytes, offsets 0, 4, 8, 12, 16, 20, 32");
static_assert(SFL_VIEW_MAX_STOPS == sfl::kViewMaxStops, "the header's limit is the kernels'");

namespace {

struct Holder {
    ViewScratch *s;
    hipStream_t stream;
    int device, dim_x, dim_y;
    size_t cells;   // of one member
    sfl::ViewFields fields;
};

Holder holder_of(sfl_context *c)
{
    return Holder{&c->views, c->stream, c->device, c->dim_x, c->gdim_y, (size_t)c->dim_x * c->gdim_y,
                  sfl::ViewFields{c->vel, c->p, c->dim_x, c->gdim_y, 1}};
}
Holder holder_of(sfl_batch *b, int first, int count)
{
    return Holder{&b->views, b->stream, b->device, b->dim_x, b->dim_y, b->cells,
                  sfl::ViewFields{b->vel + 2 * (size_t)first * b->cells, b->p + (size_t)first * b->cells, b->dim_x, b->dim_y, count}};
}

// ---- the checks that need no object ------------------------------------------------------------------------------
int check_what(const char *call, int what)
{
    if (what < SFL_VIEW_SPEED || what > SFL_VIEW_DIVERGENCE)
        return fail(SFL_ERR_INVALID, "%s: unknown view %d: SFL_VIEW_SPEED (0), SFL_VIEW_VORTICITY (1), SFL_VIEW_PRESSURE (2) or "
                    "SFL_VIEW_DIVERGENCE (3)", call, what);
    return SFL_OK;
}
int check_dx(const char *call, float dx)
{
    if (!std::isfinite(dx) || !(dx > 0.0f)) return fail(SFL_ERR_INVALID, "%s: dx must be finite and > 0 (got %g)", call, (double)dx);
    return SFL_OK;
}
int check_view(const char *call, const struct sfl_view *v)
{
    if (!v) return fail(SFL_ERR_INVALID, "%s: view is NULL", call);
    SFL_TRY(check_what(call, v->what));
    if (v->stops < 2 || v->stops > SFL_VIEW_MAX_STOPS)
        return fail(SFL_ERR_INVALID, "%s: stops must be 2..%d (got %d)", call, SFL_VIEW_MAX_STOPS, v->stops);
    if (!v->colours) return fail(SFL_ERR_INVALID, "%s: colours is NULL", call);
    const float range = v->hi - v->lo;
    if (!std::isfinite(range) || !(range > 0.0f))
        return fail(SFL_ERR_INVALID, "%s: hi - lo must be finite and > 0 (lo %g, hi %g)", call, (double)v->lo, (double)v->hi);
    SFL_TRY(check_dx(call, v->dx));
    for (int k = 0; k < 3; ++k)
        if (v->nan_colour[k] > SFL_VIEW_MAX_COLOUR)
            return fail(SFL_ERR_INVALID, "%s: nan_colour channel %d is 0x%08X, above SFL_VIEW_MAX_COLOUR (0xFC000000)", call, k, v->nan_colour[k]);
    for (int n = 0; n < 3 * v->stops; ++n)
        if (v->colours[n] > SFL_VIEW_MAX_COLOUR)
            return fail(SFL_ERR_INVALID, "%s: stop %d channel %d is 0x%08X, above SFL_VIEW_MAX_COLOUR (0xFC000000)", call, n / 3, n % 3,
                        v->colours[n]);
    return SFL_OK;
}
int check_scaling(const char *call, int scaling)
{
    if (scaling < 1 || scaling > 64) return fail(SFL_ERR_INVALID, "%s: scaling must be 1..64 (got %d)", call, scaling);
    return SFL_OK;
}

// ---- the checks on the object ------------------------------------------------------------------------------------
int check_handle(const char *call, sfl_context *c)
{
    if (!c) return fail(SFL_ERR_INVALID, "%s: ctx is NULL", call);
    if (c->nranks != 1) return fail(SFL_ERR_STATE, "%s: render needs a whole-domain context (slab %d/%d)", call, c->rank, c->nranks);
    return SFL_OK;
}
int check_range(const char *call, sfl_batch *b, int first, int count)
{
    if (!b) return fail(SFL_ERR_INVALID, "%s: batch is NULL", call);
    if (first < 0 || count < 0 || (int64_t)first + count > b->batch)
        return fail(SFL_ERR_INVALID, "%s: members [%d, %d + %d) are not inside the batch's [0, %d)", call, first, first, count, b->batch);
    return SFL_OK;
}
// the divergence view is calculate_divergence of a grid without solid cells (include/sfl.h "SOLIDS"): refused on a batch
// that has solids set, after the call's own argument checks
int check_solids(const char *call, const sfl_batch *b, int what)
{
    if (what == SFL_VIEW_DIVERGENCE && b->solids.set)
        return fail(SFL_ERR_STATE, "%s: the batch has solid cells set (sfl_batch_set_solids) and the divergence view does not know them; "
                    "sfl_batch_flow_stats reports the divergence by the solids' rule, the other views work as ever", call);
    if (what == SFL_VIEW_DIVERGENCE && b->openings.set)   // (include/sfl.h "OPENINGS")
        return fail(SFL_ERR_STATE, "%s: the batch has openings set (sfl_batch_set_openings) and the divergence view does not know them; "
                    "sfl_batch_flow_stats reports the divergence by the openings' rule, the other views work as ever", call);
    return SFL_OK;
}
// ... and on a context that has solids set (include/sfl.h "SOLIDS OF A CONTEXT")
int check_solids(const char *call, const sfl_context *c, int what)
{
    if (what == SFL_VIEW_DIVERGENCE && c->solids.set)
        return fail(SFL_ERR_STATE, "%s: the context has solid cells set (sfl_set_solids) and the divergence view does not know them; "
                    "sfl_flow_stats reports the divergence by the solids' rule, the other views work as ever", call);
    if (what == SFL_VIEW_DIVERGENCE && c->openings.set)   // (include/sfl.h "OPENINGS OF A CONTEXT")
        return fail(SFL_ERR_STATE, "%s: the context has openings set (sfl_set_openings) and the divergence view does not know them; "
                    "sfl_flow_stats reports the divergence by the openings' rule, the other views work as ever", call);
    return SFL_OK;
}
int check_bytes(const char *call, const Holder &h, size_t elem, const char *of, size_t bytes)
{
    const size_t want = (size_t)h.fields.count * h.cells * elem;
    if (bytes != want)
        return fail(SFL_ERR_INVALID, "%s: the %s of %d x %d x %d nodes are %zu bytes, got %zu", call, of, h.fields.count, h.dim_y, h.dim_x,
                    want, bytes);
    return SFL_OK;
}
int check_image_bytes(const char *call, const Holder &h, int scaling, size_t bytes)
{
    const size_t w = (size_t)scaling * (h.dim_y - 1), ht = (size_t)scaling * (h.dim_x - 1), want = (size_t)h.fields.count * ht * w * 2;
    if (bytes != want)
        return fail(SFL_ERR_INVALID, "%s: %d images of %zu x %zu uint16 are %zu bytes, got %zu", call, h.fields.count, ht, w, want, bytes);
    if (ht * w > (size_t)INT_MAX)   // (a context; a batch member has at most 20224 cells)
        return fail(SFL_ERR_INVALID, "%s: an image of %zu x %zu pixels exceeds the 2^31 - 1 pixels the render addresses inside one image", call, ht, w);
    return SFL_OK;
}

// the fields a context would hand out at this moment (as sfl_flow_stats settles them); a batch always holds its own
int settle(sfl_context *c, int what)
{
    SFL_TRY(settle_color(c, true));
    SFL_TRY(check_wait_error(c));
    SFL_TRY(ensure_field(c, what == SFL_VIEW_PRESSURE ? SFL_FIELD_PRESSURE : SFL_FIELD_VELOCITY));
    return SFL_OK;
}

// ---- staging -----------------------------------------------------------------------------------------------------
// the palette as the kernels read it: nan_colour, then the stops
std::vector<uint32_t> palette_words(const struct sfl_view *v)
{
    std::vector<uint32_t> w(v->nan_colour, v->nan_colour + 3);
    w.insert(w.end(), v->colours, v->colours + 3 * (size_t)v->stops);
    return w;
}

sfl::ViewParams params_of(const struct sfl_view *v, const uint32_t *d_palette)
{
    // 1 / (2 dx) as finitediff.cpp:36 forms it; r as include/sfl.h states it
    return sfl::ViewParams{v->what, 1.0f / (2.0f * v->dx), v->lo, 1.0f / (v->hi - v->lo), v->stops, d_palette};
}

int device_alloc(void **mem, size_t bytes, const char *what)
{
    const hipError_t e = hipMalloc(mem, bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();   // (so that the next launch's check does not report this failure again)
        return fail(e == hipErrorOutOfMemory ? SFL_ERR_NOMEM : SFL_ERR_HIP, "hipMalloc of %zu bytes of %s failed: %s", bytes, what,
                    hipGetErrorString(e));
    }
    return SFL_OK;
}

// the result's device buffer stays with the object and only grows (the calls are synchronous: it is never in flight here)
int grow_out(const Holder &h, size_t bytes)
{
    ViewScratch &s = *h.s;
    if (bytes <= s.out_bytes) return SFL_OK;
    if (s.d_out) (void)hipFree(s.d_out);
    s.d_out = nullptr;
    s.out_bytes = 0;
    SFL_TRY(device_alloc(&s.d_out, bytes, "a view's result"));
    s.out_bytes = bytes;
    return SFL_OK;
}

// the call's palette to the object's staging buffer, on its stream; `words` must live until the stream is drained
int stage_palette(const Holder &h, const std::vector<uint32_t> &words)
{
    ViewScratch &s = *h.s;
    if (!s.d_palette) SFL_TRY(device_alloc((void **)&s.d_palette, sizeof(uint32_t) * sfl::kViewPaletteWords, "a view's palette"));
    HIP_TRY(hipMemcpyAsync(s.d_palette, words.data(), words.size() * sizeof(uint32_t), hipMemcpyHostToDevice, h.stream));
    return SFL_OK;
}

// launch(d_out) on the holder's stream, then the result to the host; one wait
template <class Launch>
int produce(const Holder &h, void *host, size_t bytes, Launch launch)
{
    SFL_TRY(grow_out(h, bytes));
    HIP_TRY(launch(h.s->d_out));
    HIP_TRY(hipMemcpyAsync(host, h.s->d_out, bytes, hipMemcpyDeviceToHost, h.stream));
    HIP_TRY(hipStreamSynchronize(h.stream));   // the caller reads `host` on return
    return SFL_OK;
}

int scalar(const Holder &h, int what, float dx, float *host, size_t bytes)
{
    HIP_TRY(hipSetDevice(h.device));
    const float two_dx_inv = 1.0f / (2.0f * dx);   // finitediff.cpp:36
    return produce(h, host, bytes, [&](void *out) { return sfl::launch_view_scalar(h.stream, static_cast<float *>(out), h.fields, what, two_dx_inv); });
}

int texels(const Holder &h, const struct sfl_view *view, uint32_t *host, size_t bytes)
{
    HIP_TRY(hipSetDevice(h.device));
    const std::vector<uint32_t> words = palette_words(view);
    SFL_TRY(stage_palette(h, words));
    const sfl::ViewParams prm = params_of(view, h.s->d_palette);
    return produce(h, host, bytes, [&](void *out) { return sfl::launch_view_texels(h.stream, static_cast<uint32_t *>(out), h.fields, prm); });
}

int render(const Holder &h, const struct sfl_view *view, int scaling, int byteswap, uint16_t *host, size_t bytes)
{
    HIP_TRY(hipSetDevice(h.device));
    const std::vector<uint32_t> words = palette_words(view);
    SFL_TRY(stage_palette(h, words));
    const sfl::ViewParams prm = params_of(view, h.s->d_palette);
    return produce(h, host, bytes, [&](void *out) {
        return sfl::launch_view_render(h.stream, static_cast<uint16_t *>(out), h.fields, prm, scaling, byteswap != 0);
    });
}

// the recorder's hook (batch_frames.cpp record_step): one frame of the recorded members by the recorder's view
int record_view_frame(sfl_batch *b, uint16_t *images)
{
    const sfl_batch::Recorder &r = b->rec;
    HIP_TRY(sfl::launch_view_render(b->stream, images, holder_of(b, r.first, r.count).fields, r.view, r.scaling, r.byteswap != 0));
    return SFL_OK;
}

}  // namespace

extern "C" {

int sfl_view_scalar(sfl_context *ctx, int what, float dx, float *host, size_t bytes)
{
    const char *call = "sfl_view_scalar";
    SFL_TRY(check_what(call, what));
    SFL_TRY(check_dx(call, dx));
    SFL_TRY(check_handle(call, ctx));
    const Holder h = holder_of(ctx);
    SFL_TRY(check_bytes(call, h, sizeof(float), "scalars", bytes));
    if (!host) return fail(SFL_ERR_INVALID, "%s: host is NULL", call);
    SFL_TRY(check_solids(call, ctx, what));
    SFL_TRY(settle(ctx, what));
    return scalar(holder_of(ctx), what, dx, host, bytes);   // (settling may have swapped the context's buffers)
}

int sfl_batch_view_scalar(sfl_batch *b, int what, float dx, int first, int count, float *host, size_t bytes)
{
    const char *call = "sfl_batch_view_scalar";
    SFL_TRY(check_what(call, what));
    SFL_TRY(check_dx(call, dx));
    SFL_TRY(check_range(call, b, first, count));
    const Holder h = holder_of(b, first, count);
    SFL_TRY(check_bytes(call, h, sizeof(float), "scalars", bytes));
    SFL_TRY(check_solids(call, b, what));
    if (count == 0) return SFL_OK;
    if (!host) return fail(SFL_ERR_INVALID, "%s: host is NULL", call);
    return scalar(h, what, dx, host, bytes);
}

int sfl_view_texels(sfl_context *ctx, const struct sfl_view *view, uint32_t *host, size_t bytes)
{
    const char *call = "sfl_view_texels";
    SFL_TRY(check_view(call, view));
    SFL_TRY(check_handle(call, ctx));
    SFL_TRY(check_bytes(call, holder_of(ctx), 3 * sizeof(uint32_t), "texels", bytes));
    if (!host) return fail(SFL_ERR_INVALID, "%s: host is NULL", call);
    SFL_TRY(check_solids(call, ctx, view->what));
    SFL_TRY(settle(ctx, view->what));
    return texels(holder_of(ctx), view, host, bytes);
}

int sfl_batch_view_texels(sfl_batch *b, const struct sfl_view *view, int first, int count, uint32_t *host, size_t bytes)
{
    const char *call = "sfl_batch_view_texels";
    SFL_TRY(check_view(call, view));
    SFL_TRY(check_range(call, b, first, count));
    const Holder h = holder_of(b, first, count);
    SFL_TRY(check_bytes(call, h, 3 * sizeof(uint32_t), "texels", bytes));
    SFL_TRY(check_solids(call, b, view->what));
    if (count == 0) return SFL_OK;
    if (!host) return fail(SFL_ERR_INVALID, "%s: host is NULL", call);
    return texels(h, view, host, bytes);
}

int sfl_view_render(sfl_context *ctx, const struct sfl_view *view, int scaling, int byteswap, uint16_t *host_image, size_t bytes)
{
    const char *call = "sfl_view_render";
    SFL_TRY(check_view(call, view));
    SFL_TRY(check_scaling(call, scaling));
    SFL_TRY(check_handle(call, ctx));
    SFL_TRY(check_image_bytes(call, holder_of(ctx), scaling, bytes));
    if (!host_image) return fail(SFL_ERR_INVALID, "%s: host_image is NULL", call);
    SFL_TRY(check_solids(call, ctx, view->what));
    SFL_TRY(settle(ctx, view->what));
    return render(holder_of(ctx), view, scaling, byteswap, host_image, bytes);
}

int sfl_batch_view_render_members(sfl_batch *b, const struct sfl_view *view, int first, int count, int scaling, int byteswap,
                                  uint16_t *host_images, size_t bytes)
{
    const char *call = "sfl_batch_view_render_members";
    SFL_TRY(check_view(call, view));
    SFL_TRY(check_scaling(call, scaling));
    SFL_TRY(check_range(call, b, first, count));
    const Holder h = holder_of(b, first, count);
    SFL_TRY(check_image_bytes(call, h, scaling, bytes));
    SFL_TRY(check_solids(call, b, view->what));
    if (count == 0) return SFL_OK;
    if (!host_images) return fail(SFL_ERR_INVALID, "%s: host_images is NULL", call);
    return render(h, view, scaling, byteswap, host_images, bytes);
}

int sfl_batch_record_view(sfl_batch *b, const struct sfl_view *view)
{
    const char *call = "sfl_batch_record_view";
    if (view) SFL_TRY(check_view(call, view));
    if (!b) return fail(SFL_ERR_INVALID, "%s: batch is NULL", call);
    if (!b->rec.on) return fail(SFL_ERR_STATE, "%s: the batch is not recording: call sfl_batch_record_start first", call);
    if (!view) {   // the dye again, from the next frame on
        b->rec.view_on = false;
        return SFL_OK;
    }
    SFL_TRY(check_solids(call, b, view->what));
    HIP_TRY(hipSetDevice(b->device));
    if (!b->d_rec_palette) SFL_TRY(device_alloc((void **)&b->d_rec_palette, sizeof(uint32_t) * sfl::kViewPaletteWords, "the recorder's palette"));
    // The copy is ordered on the stream behind the frames that read the palette it replaces.  Its source is the batch's
    // own host copy, not the caller's memory (a copy from pageable memory has read its source when the call returns:
    // the next call may assign the vector anew)
    b->rec_palette_host = palette_words(view);
    HIP_TRY(hipMemcpyAsync(b->d_rec_palette, b->rec_palette_host.data(), b->rec_palette_host.size() * sizeof(uint32_t),
                           hipMemcpyHostToDevice, b->stream));
    b->rec.view = params_of(view, b->d_rec_palette);
    b->rec.view_on = true;
    b->record_view_frame = record_view_frame;
    return SFL_OK;
}

}  // extern "C"
