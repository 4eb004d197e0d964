// field_view.hip -- the flow itself as pictures (include/sfl.h "VIEWS"; gfx950 / MI355X): speed, vorticity, pressure and
// divergence of a context or of many members of a batch, as scalar fields, as node colours (the scalar through a
// palette) and as RGB565 images of those colours, drawn by the draw task's own chain.
//
// One statement of each piece, shared by the two kernels:
//   node_scalar   the four scalars from a node's 3 x 3 neighbourhood, laid out as flow_stats.hip lays it out for
//                 advect_math.h's divergence_sum -- the divergence IS that function times 1 / (2 dx), the vorticity
//                 is the definition of include/sfl.h (a neighbour outside the domain = minus the node's own component);
//   view_texel    scalar -> palette position -> the lerp of two stops, narrowed to UQ32 per channel.
//
// view_field_kernel: scalars or texels in ONE streaming pass over members x nodes.  An item is 256 consecutive nodes of
//   one member, lanes along i (the fields' fast axis): the centre loads of a wave are contiguous, the neighbours come from
//   the same and the two adjacent rows (cache).  Items are dealt to at most kMaxGrid workgroups that stride over them; the
//   member base is formed in 64-bit, the offset inside a member is 32-bit (a context has at most 2^28 cells).  The palette
//   is staged in LDS once per workgroup.  No atomics.
//
// view_render_kernel: batch_render.hip's tile scheme (render_tile.h) with another load phase.  Per tile of 16 x 32 blocks:
//   window  the velocity (or the pressure) of the tile's 17 x 33 nodes and a one-node ring, clipped at the walls, goes to
//           LDS: vx and vy as two WORD planes (not float2), node (i, j) at slot (j - j0 + 1) * kWinPitch + (i - i0 + 1).
//           Column j of the window is one contiguous span along i in memory, read with consecutive lanes along it;
//   nodes   one thread per node, lanes along i: the neighbourhood from the planes (single-word ds_read_b32s), the scalar,
//           the texel; its three channels, widened, go to the draw's LDS layout (pitch 51);
//   draw    render_tile.h draw_tile, the code batch_render_kernel runs.
//
// LDS banks (the guide's rule for ds_read_b32 / ds_write_b32: bank = word % 32, conflicts within each 32-lane half).
// This is the rule applied, not a measurement: no counter (SQ_LDS_BANK_CONFLICT) has been read for this kernel yet.
//   nodes, reads:   node n = 17 * jt + it of a full tile reads slot (jt + 1) * 49 + it + 1, and 49 = 17 (mod 32), so the
//                   slot is n + 18 (mod 32): 32 consecutive nodes -> 32 banks; the four neighbours are the same map
//                   shifted by +-1 and +-49, the second plane by kPlane: no conflict.  kWinPitch = 49 is the smallest
//                   pitch >= 19 (the window's width) that is 17 (mod 32);
//   nodes, writes:  channel k of node n goes to word 51 * jt + 3 * it + k = 3 n + k, and 3 is odd: 32 consecutive nodes
//                   -> 32 banks, for each k;
//   window, writes: lane w of a column's span writes plane w & 1, slot base + (w >> 1); kPlane = 16 (mod 32) puts the two
//                   planes 16 banks apart, so 32 consecutive words of one span -> 32 banks.  Where a span ends inside a
//                   half (38 words per column) its last words and the next column's first can meet two to a bank;
//   a tile cut by the domain's edge (rows < 16) loses the n -> bank identity: conflicts there, on edge tiles only;
//   palette:        a gather by the node's value: lanes with the same stop read the same words (a broadcast), lanes with
//                   different stops may conflict; nothing to lay out.
//   draw:           batch_render.hip's argument, unchanged.
//
// Numerics contract: -ffp-contract=off, every product, sum and quotient rounded on its own.
#include <algorithm>

#include "../../include/sfl.h"
#include "render_tile.h"
#include "view_kernels.h"

namespace sfl {
namespace {

using namespace render_tile;
using advect_math::uq_narrow;
using advect_math::uq_widen;

constexpr int kWinPitch = 49;    // words per staged window column (see above)
constexpr int kWinCols = kTileJ + 3;
constexpr int kPlane = 1744;     // words from the vx plane to the vy plane: >= kWinCols * kWinPitch, 16 (mod 32)
static_assert(kWinPitch >= kTileI + 3 && kWinPitch % 32 == (kTileI + 1) % 32, "node n of a full tile reads bank n + const");
static_assert(kPlane >= kWinCols * kWinPitch && kPlane % 32 == 16, "the planes lie 16 banks apart");

// The scalar `what` of node (i, j).  win: the node's neighbourhood as divergence_sum addresses it -- rows 3 apart, the node
// at win[4], W and E at win[3] and win[5], S and N at win[1] and win[7]; an entry the domain does not have is never read.
__device__ __forceinline__ float node_scalar(int what, const float2 (&win)[9], float pressure, int i, int j, int i_max,
                                             int j_max, float two_dx_inv)
{
    if (what == SFL_VIEW_SPEED) {
        const float xx = win[4].x * win[4].x, yy = win[4].y * win[4].y;
        return sqrtf(xx + yy);
    }
    if (what == SFL_VIEW_VORTICITY) {   // ((E - W) - (N - S)) * k; a ghost is minus the node's own component
        const float ghost_x = -win[4].x, ghost_y = -win[4].y;
        const float e = (i < i_max) ? win[5].y : ghost_y, w = (i > 0) ? win[3].y : ghost_y;
        const float n = (j < j_max) ? win[7].x : ghost_x, s = (j > 0) ? win[1].x : ghost_x;
        const float ew = e - w, ns = n - s;
        return (ew - ns) * two_dx_inv;
    }
    if (what == SFL_VIEW_PRESSURE) return pressure;
    return advect_math::divergence_sum(win + 4, 3, i, j, i_max, j_max) * two_dx_inv;
}

// The palette of a view in LDS: the stops widened (the lerp's a and b), nan_colour raw
struct Palette {
    float stop[3 * kViewMaxStops];
    uint32_t nan[3];
};

__device__ __forceinline__ void stage_palette(Palette &pal, const ViewParams &v)
{
    for (int n = threadIdx.x; n < 3 * v.stops; n += kThreads) pal.stop[n] = uq_widen(v.palette[3 + n]);
    if (threadIdx.x < 3) pal.nan[threadIdx.x] = v.palette[threadIdx.x];
}

// scalar -> texel (include/sfl.h "scalar -> texel")
__device__ __forceinline__ void view_texel(uint32_t (&out)[3], float s, const ViewParams &v, const Palette &pal)
{
    const float d = s - v.lo;
    float t = d * v.r;
    if (s != s || t != t) {
        out[0] = pal.nan[0], out[1] = pal.nan[1], out[2] = pal.nan[2];
        return;
    }
    t = t < 0.0f ? 0.0f : (t > 1.0f ? 1.0f : t);   // (+-inf included)
    const float x = t * (float)(v.stops - 1);
    const int n = min((int)x, v.stops - 2);
    const float f = x - (float)n;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float a = pal.stop[3 * n + k], b = pal.stop[3 * n + 3 + k];
        const float step = (b - a) * f;
        out[k] = uq_narrow(a + step);
    }
}

// ---- scalars and texels: one streaming pass ----------------------------------------------------------------------
template <bool TEXELS>
__global__ void __launch_bounds__(kThreads)
view_field_kernel(void *__restrict__ out, ViewFields g, ViewParams v, int items_per_member, unsigned long long items)
{
    __shared__ Palette pal;
    if (TEXELS) {
        stage_palette(pal, v);
        __syncthreads();
    }
    const int cells = g.dim_x * g.dim_y, i_max = g.dim_x - 1, j_max = g.dim_y - 1;
    for (unsigned long long item = blockIdx.x; item < items; item += gridDim.x) {
        const unsigned long long member = item / (unsigned)items_per_member;
        const int c = (int)(item - member * (unsigned)items_per_member) * kThreads + (int)threadIdx.x;
        if (c >= cells) continue;
        const unsigned long long base = member * (unsigned long long)cells;
        const int j = c / g.dim_x, i = c - j * g.dim_x;
        float2 win[9] = {};
        float pressure = 0.0f;
        if (v.what == SFL_VIEW_PRESSURE) {
            pressure = g.p[base + c];
        } else {
            const float2 *q = reinterpret_cast<const float2 *>(g.v) + base + c;
            win[4] = q[0];
            if (v.what != SFL_VIEW_SPEED) {
                if (i > 0) win[3] = q[-1];
                if (i < i_max) win[5] = q[1];
                if (j > 0) win[1] = q[-g.dim_x];
                if (j < j_max) win[7] = q[g.dim_x];
            }
        }
        const float s = node_scalar(v.what, win, pressure, i, j, i_max, j_max, v.two_dx_inv);
        if (TEXELS) {
            uint32_t t[3];
            view_texel(t, s, v, pal);
            uint32_t *o = static_cast<uint32_t *>(out) + 3 * (base + c);
            o[0] = t[0], o[1] = t[1], o[2] = t[2];
        } else {
            static_cast<float *>(out)[base + c] = s;
        }
    }
}

// ---- images ------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads)
view_render_kernel(uint16_t *__restrict__ images, ViewFields g, ViewParams v, int scaling, int byteswap, int tiles_i,
                   int tiles_j, unsigned long long total)
{
    __shared__ float window[2 * kPlane];
    __shared__ float texel[kTexelWords];
    __shared__ Palette pal;
    stage_palette(pal, v);   // (read behind the first tile's barrier)
    const int dim_x = g.dim_x, dim_y = g.dim_y, i_max = dim_x - 1, j_max = dim_y - 1;
    const int tiles = tiles_i * tiles_j;
    const int width = scaling * (dim_y - 1), height = scaling * (dim_x - 1);
    const float inv = render_math::render_inv(scaling);
    const bool scalar_field = v.what == SFL_VIEW_PRESSURE;   // one word per node, one plane
    for (unsigned long long wg = blockIdx.x; wg < total; wg += gridDim.x) {
        const unsigned long long member = wg / (unsigned)tiles;
        const int tile = (int)(wg - member * (unsigned)tiles);
        const int ti = tile % tiles_i, tj = tile / tiles_i;
        const int i0 = ti * kTileI, j0 = tj * kTileJ;
        const int rows = min(kTileI, dim_x - 1 - i0), cols = min(kTileJ, dim_y - 1 - j0);   // cell blocks of this tile
        const unsigned long long base = member * (unsigned long long)dim_x * (unsigned long long)dim_y;
        uint16_t *image = images + member * (unsigned long long)height * (unsigned long long)width;

        // window: nodes [wi0, wi1] x [wj0, wj1] = the tile's and their ring, clipped at the walls; node (i, j) at slot
        // (j - j0 + 1) * kWinPitch + (i - i0 + 1): slots 0 .. rows + 2 of columns 0 .. cols + 2
        const int wi0 = max(i0 - 1, 0), wi1 = min(i0 + rows + 1, i_max), wj0 = max(j0 - 1, 0), wj1 = min(j0 + cols + 1, j_max);
        const int ni = wi1 - wi0 + 1, nj = wj1 - wj0 + 1;
        const int slot0 = (wj0 - j0 + 1) * kWinPitch + (wi0 - i0 + 1);
        if (scalar_field) {
            const float *p = g.p + base;
            for (int n = threadIdx.x; n < nj * ni; n += kThreads) {
                const int jw = n / ni, w = n - jw * ni;
                window[slot0 + jw * kWinPitch + w] = p[dim_x * (wj0 + jw) + wi0 + w];
            }
        } else {
            const float *vel = g.v + 2 * base;
            const int span = 2 * ni;
            for (int n = threadIdx.x; n < nj * span; n += kThreads) {
                const int jw = n / span, w = n - jw * span;
                window[(w & 1) * kPlane + slot0 + jw * kWinPitch + (w >> 1)] = vel[2 * (dim_x * (wj0 + jw) + wi0) + w];
            }
        }
        __syncthreads();

        // nodes: scalar -> texel, widened into the draw's layout
        const int span_i = rows + 1;
        for (int n = threadIdx.x; n < (cols + 1) * span_i; n += kThreads) {
            const int jt = n / span_i, it = n - jt * span_i;
            const int i = i0 + it, j = j0 + jt;
            const float *x = window + (jt + 1) * kWinPitch + it + 1, *y = x + kPlane;
            float2 win[9] = {};
            float pressure = 0.0f;
            if (scalar_field) {
                pressure = x[0];
            } else {
                win[4] = make_float2(x[0], y[0]);
                if (v.what != SFL_VIEW_SPEED) {
                    if (i > 0) win[3] = make_float2(x[-1], y[-1]);
                    if (i < i_max) win[5] = make_float2(x[1], y[1]);
                    if (j > 0) win[1] = make_float2(x[-kWinPitch], y[-kWinPitch]);
                    if (j < j_max) win[7] = make_float2(x[kWinPitch], y[kWinPitch]);
                }
            }
            uint32_t t[3];
            view_texel(t, node_scalar(v.what, win, pressure, i, j, i_max, j_max, v.two_dx_inv), v, pal);
            float *o = texel + jt * kPitch + 3 * it;
            o[0] = uq_widen(t[0]), o[1] = uq_widen(t[1]), o[2] = uq_widen(t[2]);
        }
        __syncthreads();

        draw_tile(texel, image, i0, j0, rows, cols, scaling, width, inv, byteswap);
        __syncthreads();   // the next tile's phases overwrite what this one's read
    }
}

}  // namespace

static hipError_t launch_field(hipStream_t s, void *out, const ViewFields &f, const ViewParams &v, bool texels)
{
    if (f.count <= 0 || f.dim_x < 2 || f.dim_y < 2) return hipSuccess;
    const long long cells = (long long)f.dim_x * f.dim_y;
    const int items_per_member = (int)((cells + kThreads - 1) / kThreads);
    const unsigned long long items = (unsigned long long)f.count * (unsigned)items_per_member;
    const unsigned grid = (unsigned)std::min<unsigned long long>(items, kMaxGrid);
    if (texels)
        view_field_kernel<true><<<grid, kThreads, 0, s>>>(out, f, v, items_per_member, items);
    else
        view_field_kernel<false><<<grid, kThreads, 0, s>>>(out, f, v, items_per_member, items);
    return hipGetLastError();
}

hipError_t launch_view_scalar(hipStream_t s, float *out, const ViewFields &f, int what, float two_dx_inv)
{
    return launch_field(s, out, f, ViewParams{what, two_dx_inv, 0.0f, 1.0f, 2, nullptr}, false);
}

hipError_t launch_view_texels(hipStream_t s, uint32_t *out, const ViewFields &f, const ViewParams &v)
{
    return launch_field(s, out, f, v, true);
}

hipError_t launch_view_render(hipStream_t s, uint16_t *images, const ViewFields &f, const ViewParams &v, int scaling,
                              bool byteswap)
{
    if (f.count <= 0 || f.dim_x < 2 || f.dim_y < 2 || scaling < 1) return hipSuccess;
    const int tiles_i = (f.dim_x - 1 + kTileI - 1) / kTileI, tiles_j = (f.dim_y - 1 + kTileJ - 1) / kTileJ;
    const unsigned long long total = (unsigned long long)f.count * (unsigned)tiles_i * (unsigned)tiles_j;
    const unsigned grid = (unsigned)(total < kMaxGrid ? total : kMaxGrid);
    view_render_kernel<<<grid, kThreads, 0, s>>>(images, f, v, scaling, byteswap ? 1 : 0, tiles_i, tiles_j, total);
    return hipGetLastError();
}

}  // namespace sfl
