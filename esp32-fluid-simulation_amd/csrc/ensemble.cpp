// ensemble.cpp -- what an ensemble is run for, without downloading its fields (include/sfl.h groups 2 and 4): the distance
// between two contexts (sfl_distance) or between the members of batches (sfl_batch_distance) -- maxima of |a - b|, exact
// dye sums, the number of cells whose bits differ -- and the per-cell envelope of the dye over the members of a batch
// (sfl_batch_envelope*: mean, minimum, maximum, spread).  Host C++ only; the kernels are field_distance.hip and
// batch_envelope.hip (ensemble_kernels.h), the draw kernel of the envelope's pictures is batch_render.hip's.  Every call
// only READS the fields: no validity flag, timeline or recorder of a context or batch is touched here.
#include "batch_state.h"
#include "ensemble_kernels.h"

using namespace sfl::host;

static_assert(sizeof(struct sfl_field_distance) == 64 && offsetof(struct sfl_field_distance, max_abs_dp) == 8 &&
                  offsetof(struct sfl_field_distance, what) == 12 && offsetof(struct sfl_field_distance, velocity_cells_differ) == 16 &&
                  offsetof(struct sfl_field_distance, dye_cells_differ) == 20 && offsetof(struct sfl_field_distance, pressure_cells_differ) == 24 &&
                  offsetof(struct sfl_field_distance, max_abs_ddye) == 28 && offsetof(struct sfl_field_distance, sum_abs_ddye) == 40,
              "sfl_field_distance: 64 bytes, offsets 0, 4, 8, 12, 16, 20, 24, 28, 40");

namespace {

constexpr int kDistAll = SFL_DIST_VELOCITY | SFL_DIST_DYE | SFL_DIST_PRESSURE;

int check_what(int what)   // (first: it needs no handle to be wrong)
{
    if (what == 0 || (what & ~kDistAll))
        return fail(SFL_ERR_INVALID, "what must be a non-empty set of SFL_DIST_VELOCITY (1), SFL_DIST_DYE (2) and SFL_DIST_PRESSURE (4) (got %d)", what);
    return SFL_OK;
}

int check_which(int which)
{
    if (which < SFL_ENV_MEAN || which > SFL_ENV_SPREAD)
        return fail(SFL_ERR_INVALID, "which must be SFL_ENV_MEAN (0), SFL_ENV_MIN (1), SFL_ENV_MAX (2) or SFL_ENV_SPREAD (3) (got %d)", which);
    return SFL_OK;
}

int use_device(sfl_batch *b)
{
    HIP_TRY(hipSetDevice(b->device));
    return SFL_OK;
}

// the fields a context would hand out at this moment (as sfl_flow_stats settles them, the pressure as sfl_download's)
int settle_fields(sfl_context *c, int what)
{
    SFL_TRY(settle_color(c, true));
    SFL_TRY(check_wait_error(c));
    if (what & SFL_DIST_VELOCITY) SFL_TRY(ensure_field(c, SFL_FIELD_VELOCITY));
    if (what & SFL_DIST_DYE) SFL_TRY(ensure_field(c, SFL_FIELD_COLOR));
    if (what & SFL_DIST_PRESSURE) SFL_TRY(ensure_field(c, SFL_FIELD_PRESSURE));
    return SFL_OK;
}

// member m of a batch as one side of a distance; stride 0: every record against that member
sfl::DistanceSide side_of(const sfl_batch *b, int m, bool fixed)
{
    const size_t at = (size_t)m * b->cells;
    return sfl::DistanceSide{b->vel + 2 * at, b->col + 3 * at, b->p + at, fixed ? 0 : b->cells};
}

size_t member_words(const sfl_batch *b) { return 3 * b->cells; }

}  // namespace

extern "C" {

int sfl_distance(sfl_context *a, sfl_context *b, int what, struct sfl_field_distance *out)
{
    SFL_TRY(check_what(what));
    if (!a || !b || !out) return fail(SFL_ERR_INVALID, "NULL argument");
    for (const sfl_context *c : {a, b})
        if (c->nranks != 1)   // (a slab's figures would need a reduction over the ranks)
            return fail(SFL_ERR_STATE, "sfl_distance: whole-domain contexts only (slab %d/%d)", c->rank, c->nranks);
    if (a->dim_x != b->dim_x || a->gdim_y != b->gdim_y)
        return fail(SFL_ERR_INVALID, "sfl_distance: a is %d x %d and b is %d x %d: the shapes must be the same", a->dim_x, a->gdim_y,
                    b->dim_x, b->gdim_y);
    if (a->device != b->device)
        return fail(SFL_ERR_INVALID, "sfl_distance: a is on device %d and b on device %d: they must share one", a->device, b->device);
    SFL_TRY(settle_fields(a, what));
    if (b != a) SFL_TRY(settle_fields(b, what));
    SFL_TRY(use_device(a));
    if (!a->d_dist) HIP_TRY(hipMalloc((void **)&a->d_dist, sizeof(struct sfl_field_distance)));
    if (!a->h_dist) HIP_TRY(hipHostMalloc((void **)&a->h_dist, sizeof(struct sfl_field_distance), hipHostMallocDefault));
    if (b != a) HIP_TRY(hipStreamSynchronize(b->stream));   // what b's stream still writes is read here
    const size_t cells = (size_t)a->dim_x * a->gdim_y;
    const sfl::DistanceSide sa{a->vel, a->col, a->p, cells}, sb{b->vel, b->col, b->p, cells};
    HIP_TRY(sfl::launch_field_distance(a->stream, reinterpret_cast<sfl::DistanceRecord *>(a->d_dist), what, sa, sb, cells, 1));
    HIP_TRY(hipMemcpyAsync(a->h_dist, a->d_dist, sizeof(struct sfl_field_distance), hipMemcpyDeviceToHost, a->stream));
    HIP_TRY(hipStreamSynchronize(a->stream));
    *out = *a->h_dist;
    out->what = (uint32_t)what;
    return SFL_OK;
}

int sfl_batch_distance(sfl_batch *b, int what, sfl_batch *ref, int ref_member, int first, int count,
                       struct sfl_field_distance *host, size_t bytes)
{
    SFL_TRY(check_what(what));
    if (count < 0 || bytes != (size_t)count * sizeof(struct sfl_field_distance))
        return fail(SFL_ERR_INVALID, "the distance records of %d members are %zu bytes, got %zu", count,
                    (size_t)std::max(count, 0) * sizeof(struct sfl_field_distance), bytes);
    if (!b || !host) return fail(SFL_ERR_INVALID, "NULL argument");
    if (!ref) ref = b;
    if (first < 0 || (int64_t)first + count > b->batch)
        return fail(SFL_ERR_INVALID, "members [%d, %d + %d) are not inside the batch's [0, %d)", first, first, count, b->batch);
    if (ref_member < -1 || ref_member >= ref->batch)
        return fail(SFL_ERR_INVALID, "ref_member %d is not -1 (pairwise) or inside the reference batch's [0, %d)", ref_member, ref->batch);
    if (ref_member == -1 && (int64_t)first + count > ref->batch)
        return fail(SFL_ERR_INVALID, "pairwise: members [%d, %d + %d) are not inside the reference batch's [0, %d)", first, first, count,
                    ref->batch);
    if (ref->dim_x != b->dim_x || ref->dim_y != b->dim_y)
        return fail(SFL_ERR_INVALID, "the batch's members are %d x %d and the reference's %d x %d: the shapes must be the same", b->dim_x,
                    b->dim_y, ref->dim_x, ref->dim_y);
    if (ref->device != b->device)
        return fail(SFL_ERR_INVALID, "the batch is on device %d and the reference on device %d: they must share one", b->device, ref->device);
    if (count == 0) return SFL_OK;
    SFL_TRY(use_device(b));
    const size_t all_bytes = sizeof(struct sfl_field_distance) * (size_t)b->batch;
    if (!b->d_dist) HIP_TRY(hipMalloc((void **)&b->d_dist, all_bytes));
    if (!b->h_dist) HIP_TRY(hipHostMalloc((void **)&b->h_dist, all_bytes, hipHostMallocDefault));
    if (ref != b) HIP_TRY(hipStreamSynchronize(ref->stream));   // what ref's stream still writes is read here
    // (the call is synchronous: the pinned block is never in flight when the next call writes it)
    const sfl::DistanceSide sa = side_of(b, first, false);
    const sfl::DistanceSide sr = ref_member >= 0 ? side_of(ref, ref_member, true) : side_of(ref, first, false);
    HIP_TRY(sfl::launch_field_distance(b->stream, reinterpret_cast<sfl::DistanceRecord *>(b->d_dist), what, sa, sr, b->cells, count));
    HIP_TRY(hipMemcpyAsync(b->h_dist, b->d_dist, bytes, hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    memcpy(host, b->h_dist, bytes);
    for (int k = 0; k < count; ++k) host[k].what = (uint32_t)what;
    return SFL_OK;
}

int sfl_batch_envelope(sfl_batch *b, int first, int count)
{
    if (!b) return fail(SFL_ERR_INVALID, "batch is NULL");
    if (count < 1) return fail(SFL_ERR_INVALID, "count must be >= 1 (got %d)", count);
    if (first < 0 || (int64_t)first + count > b->batch)
        return fail(SFL_ERR_INVALID, "members [%d, %d + %d) are not inside the batch's [0, %d)", first, first, count, b->batch);
    SFL_TRY(use_device(b));
    const size_t words = member_words(b);
    if (!b->d_env) {   // the four fields and the partials of the largest range there can be: once per batch
        const size_t bytes = sizeof(uint32_t) * (4 * words + sfl::envelope_partial_words(b->batch, words));
        HIP_TRY(hipMalloc((void **)&b->d_env, bytes));
    }
    // (downloads and renders of the snapshot this one replaces are synchronous: none is in flight)
    HIP_TRY(sfl::launch_batch_envelope(b->stream, b->d_env, b->d_env + 4 * words, b->col + (size_t)first * words, words, count));
    b->env_first = first;
    b->env_count = count;
    return SFL_OK;
}

int sfl_batch_envelope_info(sfl_batch *b, int *first, int *count)
{
    if (!b) return fail(SFL_ERR_INVALID, "batch is NULL");
    if (first) *first = b->env_first;
    if (count) *count = b->env_count;
    return SFL_OK;
}

int sfl_batch_envelope_download(sfl_batch *b, int which, uint32_t *host, size_t bytes)
{
    SFL_TRY(check_which(which));
    if (b && bytes != member_words(b) * sizeof(uint32_t))
        return fail(SFL_ERR_INVALID, "a field of the envelope is %zu bytes, got %zu", member_words(b) * sizeof(uint32_t), bytes);
    if (!b || !host) return fail(SFL_ERR_INVALID, "NULL argument");
    if (b->env_count == 0) return fail(SFL_ERR_STATE, "the batch holds no envelope yet: call sfl_batch_envelope first");
    SFL_TRY(use_device(b));
    HIP_TRY(hipMemcpyAsync(host, b->d_env + (size_t)which * member_words(b), bytes, hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return SFL_OK;
}

int sfl_batch_envelope_render(sfl_batch *b, int which, int scaling, int byteswap, uint16_t *host_image, size_t bytes)
{
    SFL_TRY(check_which(which));
    if (scaling < 1 || scaling > 64) return fail(SFL_ERR_INVALID, "scaling must be 1..64 (got %d)", scaling);
    if (b) {
        const size_t w = (size_t)scaling * (b->dim_y - 1), h = (size_t)scaling * (b->dim_x - 1), want = h * w * 2;
        if (bytes != want) return fail(SFL_ERR_INVALID, "an image of %zu x %zu uint16 is %zu bytes, got %zu", h, w, want, bytes);
    }
    if (!b || !host_image) return fail(SFL_ERR_INVALID, "NULL argument");
    if (b->env_count == 0) return fail(SFL_ERR_STATE, "the batch holds no envelope yet: call sfl_batch_envelope first");
    SFL_TRY(use_device(b));
    if (bytes > b->d_image_bytes) {   // the batch's single-image buffer (sfl_batch_render_rgb565 keeps it too); every user is synchronous
        if (b->d_image) (void)hipFree(b->d_image);
        b->d_image = nullptr;
        b->d_image_bytes = 0;
        HIP_TRY(hipMalloc((void **)&b->d_image, bytes));
        b->d_image_bytes = bytes;
    }
    HIP_TRY(sfl::launch_batch_render(b->stream, b->d_image, b->d_env + (size_t)which * member_words(b), b->dim_x, b->dim_y, 1, scaling,
                                     byteswap != 0));
    HIP_TRY(hipMemcpyAsync(host_image, b->d_image, bytes, hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));   // the caller reads host_image on return
    return SFL_OK;
}

}  // extern "C"
