// batch_render.hip -- the draw task (ino:116-176) of many members of a batch in ONE launch, for gfx950 (MI355X).
//
// An image's fast axis (j, across the screen) is the dye's slow one: texel (i, j) of a member is at 3 * (dim_x * j + i),
// so a kernel with one thread per pixel and lanes along the image row (stencil_kernels.hip render_rgb565_kernel) reads
// with a stride of 12 * dim_x bytes between lanes and fetches every texel about scaling^2 times.  Here the render is
// the LDS transpose it is:
//
//   * one workgroup renders one tile of kTileI x kTileJ cell blocks of one member;
//   * load: the tile's (kTileI + 1) x (kTileJ + 1) corner texels, widened to float, go to LDS.  A column j of the tile is
//     ONE contiguous span of 3 * (rows + 1) words in global memory (i is the dye's fast axis), read with consecutive lanes
//     along it.  A texel is fetched once per tile that touches it (the one-texel overlap with the neighbour included);
//   * draw: consecutive lanes run along the image row, one thread per block and image row: it takes the block's four
//     corners from LDS, walks both edges once and then across its `scaling` pixels by the chain of render_math.h (the
//     chain of a pixel is a prefix of its right neighbour's), and stores them, in pairs where they are aligned.  The
//     tile's constants and this phase live in render_tile.h: field_view.hip draws its node colours with the same code.
//
// LDS layout: word 3 * it + k of column jt at jt * kPitch, kPitch = 3 * (kTileI + 1) = 51 words, no padding.  The guide's
// bank rule (section 2) for ds_write_b32 / ds_read_b32: bank = word % 32, conflicts within each 32-lane half.  The
// compiler pairs some of the draw's reads of neighbouring corner words into ds_read2_b32, which bank as two ds_read_b32:
// the argument below holds for each of the two.  This is the rule applied, not a measurement: no counter
// (SQ_LDS_BANK_CONFLICT) has been read for this kernel yet.
//   load:  a half's lanes write 32 consecutive words (a full column's end continues at the next column's start: kPitch
//          is its length; a tile cut by the domain's edge leaves a gap there) -> 32 banks, no conflict;
//   draw:  a half's lanes read word jt * 51 + c with one c (a full tile: the 32 blocks of one image row) and 32
//          consecutive jt.  51 is odd, so jt -> jt * 51 mod 32 is one-to-one on them: no conflict, for either corner
//          column (jt and jt + 1) and every k.  (A tile cut to fewer than 32 blocks puts several image rows into a
//          half: rows of one `it` read the same words, a broadcast; rows of two `it` can meet on a bank.  Edge tiles
//          only.)
//
// Addressing: a member's dye and image bases are formed in 64-bit (a frame of many members exceeds 2^32 bytes); offsets
// inside one member stay 32-bit (at most 20224 cells x 64^2 pixels).  Members and tiles are flattened into a 1-D grid
// of at most kMaxGrid workgroups that stride over the pairs, so no grid dimension limits the number of members.  A
// member's image starts on a 2-byte boundary only (H * W can be odd): every 32-bit store checks its own alignment, the
// rest are 16-bit.
#include "batch.h"
#include "render_tile.h"

namespace sfl {
namespace {

using namespace render_math;
using namespace render_tile;   // the tile's constants and its draw phase, shared with field_view.hip
using advect_math::uq_widen;

__global__ void __launch_bounds__(kThreads)
batch_render_kernel(uint16_t *__restrict__ images, const uint32_t *__restrict__ colour, int dim_x, int dim_y, int scaling,
                    int byteswap, int tiles_i, int tiles_j, unsigned long long total)
{
    __shared__ float texel[kTexelWords];
    const int tiles = tiles_i * tiles_j;
    const int width = scaling * (dim_y - 1), height = scaling * (dim_x - 1);
    const float inv = render_inv(scaling);
    for (unsigned long long wg = blockIdx.x; wg < total; wg += gridDim.x) {
        const unsigned long long member = wg / (unsigned)tiles;
        const int tile = (int)(wg - member * (unsigned)tiles);
        const int ti = tile % tiles_i, tj = tile / tiles_i;   // (neighbours in i share cache lines of the columns)
        const int i0 = ti * kTileI, j0 = tj * kTileJ;
        const int rows = min(kTileI, dim_x - 1 - i0), cols = min(kTileJ, dim_y - 1 - j0);   // cell blocks of this tile
        const uint32_t *dye = colour + 3ull * member * (unsigned long long)dim_x * (unsigned long long)dim_y;
        uint16_t *image = images + member * (unsigned long long)height * (unsigned long long)width;

        // load: columns j0 .. j0 + cols, words 3 * i0 .. 3 * (i0 + rows) + 2 of each
        const int span = 3 * (rows + 1);
        for (int n = threadIdx.x; n < (cols + 1) * span; n += kThreads) {
            const int jt = n / span, w = n - jt * span;
            texel[jt * kPitch + w] = uq_widen(dye[3 * (dim_x * (j0 + jt) + i0) + w]);
        }
        __syncthreads();

        // draw (render_tile.h): rows * scaling image rows of cols blocks; one thread takes the `scaling` pixels of one
        // block in one image row: both edge walks once, then ONE walk across (pixel jj + 1 continues the chain of pixel jj)
        draw_tile(texel, image, i0, j0, rows, cols, scaling, width, inv, byteswap);
        __syncthreads();   // the next tile's load overwrites what this one's draw reads
    }
}

}  // namespace

hipError_t launch_batch_render(hipStream_t s, uint16_t *images, const uint32_t *colour_of_first_member, int dim_x, int dim_y,
                               int count, int scaling, bool byteswap)
{
    if (count <= 0 || dim_x < 2 || dim_y < 2 || scaling < 1) return hipSuccess;
    const int tiles_i = (dim_x - 1 + kTileI - 1) / kTileI, tiles_j = (dim_y - 1 + kTileJ - 1) / kTileJ;
    const unsigned long long total = (unsigned long long)count * (unsigned)tiles_i * (unsigned)tiles_j;
    const unsigned grid = (unsigned)(total < kMaxGrid ? total : kMaxGrid);
    batch_render_kernel<<<grid, kThreads, 0, s>>>(images, colour_of_first_member, dim_x, dim_y, scaling, byteswap ? 1 : 0,
                                                  tiles_i, tiles_j, total);
    return hipGetLastError();
}

}  // namespace sfl
