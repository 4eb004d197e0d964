// batch_frames.cpp -- the draw half of a batch (include/sfl.h group 4): sfl_batch_render_members, the frames of many
// members in one launch and one copy, and the recorder sfl_batch_record_*, which renders a frame of chosen members every
// k-th step into device memory, between the step launches of sfl_batch_step_n* and on the batch's stream, so that the
// step calls stay asynchronous and the frames are read out afterwards.  Host C++ only; the kernel is batch_render.hip.
// A frame shows the dye unless sfl_batch_record_view (views.cpp) has set a view: then record_step calls through the batch's
// record_view_frame pointer, so that this unit links without the views' kernels.
#include "batch_state.h"

using sfl::host::fail;

namespace {

int use_device(sfl_batch *b)
{
    HIP_TRY(hipSetDevice(b->device));
    return SFL_OK;
}

// pixels of one member's image at a scaling
size_t image_pixels(const sfl_batch *b, int scaling)
{
    return (size_t)scaling * (b->dim_x - 1) * (size_t)scaling * (b->dim_y - 1);
}

int check_scaling(int scaling)
{
    if (scaling < 1 || scaling > 64) return fail(SFL_ERR_INVALID, "scaling must be 1..64 (got %d)", scaling);
    return SFL_OK;
}

int check_image_bytes(const sfl_batch *b, int count, int scaling, size_t bytes)
{
    const size_t w = (size_t)scaling * (b->dim_y - 1), h = (size_t)scaling * (b->dim_x - 1), want = (size_t)count * h * w * 2;
    if (bytes != want)
        return fail(SFL_ERR_INVALID, "%d images of %zu x %zu uint16 are %zu bytes, got %zu", count, h, w, want, bytes);
    return SFL_OK;
}

// a device buffer that stays with the batch and only grows; an earlier launch may still write the old one: drain on growth
int grow(sfl_batch *b, uint16_t **buf, size_t *have, size_t bytes)
{
    if (bytes <= *have) return SFL_OK;
    if (*buf) {
        HIP_TRY(hipStreamSynchronize(b->stream));
        (void)hipFree(*buf);
        *buf = nullptr;
        *have = 0;
    }
    void *mem = nullptr;
    const hipError_t e = hipMalloc(&mem, bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();   // (so that the next launch's check does not report this failure again)
        return fail(e == hipErrorOutOfMemory ? SFL_ERR_NOMEM : SFL_ERR_HIP, "hipMalloc of %zu bytes of frames failed: %s", bytes,
                    hipGetErrorString(e));
    }
    *buf = static_cast<uint16_t *>(mem);
    *have = bytes;
    return SFL_OK;
}

}  // namespace

namespace sfl {
namespace host {

int record_admit(sfl_batch *b, int n)
{
    const sfl_batch::Recorder &r = b->rec;
    if (!r.on) return SFL_OK;
    const int64_t due = (r.steps + n) / r.every - r.steps / r.every, room = r.capacity - r.written;
    if (due > room)
        return fail(SFL_ERR_STATE, "the recorder has room for %lld more frames (%d of %d written) and %d steps would complete %lld: "
                    "nothing stepped; read the frames with sfl_batch_record_read and make room with sfl_batch_record_start",
                    (long long)room, r.written, r.capacity, n, (long long)due);
    return SFL_OK;
}

int record_run(const sfl_batch *b, int n)
{
    const sfl_batch::Recorder &r = b->rec;
    if (!r.on) return n;
    return (int)std::min<int64_t>(n, r.every - r.steps % r.every);
}

int record_step(sfl_batch *b, int steps)
{
    sfl_batch::Recorder &r = b->rec;
    if (!r.on) return SFL_OK;
    r.steps += steps;
    if (r.steps % r.every != 0) return SFL_OK;
    const int frame = (int)(r.steps / r.every) - 1;   // < capacity: record_admit has let the call through
    uint16_t *images = b->d_frames + (size_t)frame * r.count * image_pixels(b, r.scaling);
    if (r.view_on && b->record_view_frame)   // (sfl_batch_record_view: the frame shows a view of v or p, not the dye)
        SFL_TRY(b->record_view_frame(b, images));
    else
        HIP_TRY(sfl::launch_batch_render(b->stream, images, b->col + 3 * (size_t)r.first * b->cells, b->dim_x, b->dim_y, r.count,
                                         r.scaling, r.byteswap != 0));
    r.written = frame + 1;
    return SFL_OK;
}

}  // namespace host
}  // namespace sfl

extern "C" {

int sfl_batch_render_members(sfl_batch *b, int first, int count, int scaling, int byteswap, uint16_t *host_images, size_t bytes)
{
    if (!b) return fail(SFL_ERR_INVALID, "batch is NULL");
    SFL_TRY(check_scaling(scaling));
    if (first < 0 || count < 0 || (int64_t)first + count > b->batch)
        return fail(SFL_ERR_INVALID, "members [%d, %d + %d) are not inside the batch's [0, %d)", first, first, count, b->batch);
    SFL_TRY(check_image_bytes(b, count, scaling, bytes));
    if (count == 0) return SFL_OK;
    if (!host_images) return fail(SFL_ERR_INVALID, "host_images is NULL");
    SFL_TRY(use_device(b));
    SFL_TRY(grow(b, &b->d_images, &b->d_images_bytes, bytes));
    HIP_TRY(sfl::launch_batch_render(b->stream, b->d_images, b->col + 3 * (size_t)first * b->cells, b->dim_x, b->dim_y, count,
                                     scaling, byteswap != 0));
    HIP_TRY(hipMemcpyAsync(host_images, b->d_images, bytes, hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));   // the caller reads host_images on return
    return SFL_OK;
}

int sfl_batch_record_start(sfl_batch *b, int every, int first, int count, int scaling, int byteswap, int capacity)
{
    if (!b) return fail(SFL_ERR_INVALID, "batch is NULL");
    if (every < 1) return fail(SFL_ERR_INVALID, "every must be >= 1 (got %d)", every);
    if (capacity < 1) return fail(SFL_ERR_INVALID, "capacity must be >= 1 (got %d)", capacity);
    SFL_TRY(check_scaling(scaling));
    if (count < 1) return fail(SFL_ERR_INVALID, "count must be >= 1 (got %d)", count);
    if (first < 0 || (int64_t)first + count > b->batch)
        return fail(SFL_ERR_INVALID, "members [%d, %d + %d) are not inside the batch's [0, %d)", first, first, count, b->batch);
    // capacity * count * H * W * 2 bytes: refused here if the product does not fit a size_t (checked by dividing)
    const size_t frame_bytes = (size_t)count * image_pixels(b, scaling) * 2;   // <= 2^31 * 20224 * 64^2 * 2 < 2^64
    if ((size_t)capacity > SIZE_MAX / frame_bytes)
        return fail(SFL_ERR_INVALID, "capacity %d frames of %zu bytes each exceed the address space", capacity, frame_bytes);
    SFL_TRY(use_device(b));
    // (renders of the recording that ends here may still be in flight: they are ahead of the new ones on the stream)
    b->rec = sfl_batch::Recorder{};   // not recording unless the frames are there
    SFL_TRY(grow(b, &b->d_frames, &b->d_frames_bytes, (size_t)capacity * frame_bytes));
    b->rec.on = true;
    b->rec.every = every;
    b->rec.first = first;
    b->rec.count = count;
    b->rec.scaling = scaling;
    b->rec.byteswap = byteswap != 0;
    b->rec.capacity = capacity;
    return SFL_OK;
}

int sfl_batch_record_stop(sfl_batch *b)
{
    if (!b) return fail(SFL_ERR_INVALID, "batch is NULL");
    b->rec = sfl_batch::Recorder{};
    if (!b->d_frames) return SFL_OK;
    SFL_TRY(use_device(b));
    HIP_TRY(hipStreamSynchronize(b->stream));   // a render may still write the frames
    (void)hipFree(b->d_frames);
    b->d_frames = nullptr;
    b->d_frames_bytes = 0;
    return SFL_OK;
}

int sfl_batch_record_info(sfl_batch *b, int *frames, int *capacity, int64_t *steps)
{
    if (!b) return fail(SFL_ERR_INVALID, "batch is NULL");
    if (frames) *frames = b->rec.written;
    if (capacity) *capacity = b->rec.capacity;
    if (steps) *steps = b->rec.steps;
    return SFL_OK;
}

int sfl_batch_record_read(sfl_batch *b, int frame, int first, int count, uint16_t *host, size_t bytes)
{
    if (!b) return fail(SFL_ERR_INVALID, "batch is NULL");
    const sfl_batch::Recorder &r = b->rec;
    if (!r.on) return fail(SFL_ERR_STATE, "the batch is not recording: no frames to read; call sfl_batch_record_start first");
    if (frame < 0 || frame >= r.written)
        return fail(SFL_ERR_INVALID, "frame %d outside the %d frames written so far, [0, %d)", frame, r.written, r.written);
    if (first < r.first || count < 0 || (int64_t)first + count > (int64_t)r.first + r.count)
        return fail(SFL_ERR_INVALID, "members [%d, %d + %d) are not inside the recorded [%d, %d + %d)", first, first, count, r.first,
                    r.first, r.count);
    SFL_TRY(check_image_bytes(b, count, r.scaling, bytes));
    if (count == 0) return SFL_OK;
    if (!host) return fail(SFL_ERR_INVALID, "host is NULL");
    SFL_TRY(use_device(b));
    const uint16_t *dev = b->d_frames + ((size_t)frame * r.count + (size_t)(first - r.first)) * image_pixels(b, r.scaling);
    HIP_TRY(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return SFL_OK;
}

}  // extern "C"
