// context_viscous.hip -- the implicit diffusion of the velocity of a whole-domain context (gfx950 / MI355X; include/sfl.h
// "VISCOSITY", item 3a) on a grid of ANY size: diffuse_kernel, the tile of diffuse_tile.h -- a workgroup of 1024 threads
// owns 64 x 32 cells, loads the 96 x 64 window around them into LDS (49 152 B: u alone, two floats per cell, the colours
// apart, three cells of a colour per thread), runs up to kD = 8 sweeps there and stores the owned cells to another
// buffer.  A diffusion of `sweeps` sweeps is ceil(sweeps / kD) launches (context_viscous.cpp).  A kernel of its own in a
// file of its own: every kernel that existed keeps its text and its instructions.  No atomics, no inline assembly.
//
// Numerics contract: -ffp-contract=off, every operation individually rounded in the rule's order.
#include "diffuse_tile.h"
#include "viscous_kernels.h"

namespace sfl {
namespace {

// (8 waves per SIMD = two workgroups per CU, which 2 x 49 152 B of LDS allow: 64 VGPRs with one spilled to scratch beat 67
// VGPRs and one workgroup per CU by 1.27 x -- profiles/viscosity.txt)
__global__ void __launch_bounds__(diffuse::kThreads) __attribute__((amdgpu_waves_per_eu(8)))
diffuse_kernel(diffuse::Vec2 *__restrict__ u_out, const diffuse::Vec2 *u_in, const diffuse::Vec2 *u0,
               const uint8_t *__restrict__ codes, int dim_x, int dim_y, int k, float a, float c, bool zero_solids)
{
    __shared__ diffuse::Vec2 lds[diffuse::kLdsCells];
    diffuse::Tile t;
    t.u_in = u_in;
    t.u0 = u0;
    t.u_out = u_out;
    t.codes = codes;
    t.dim_x = dim_x;
    t.dim_y = dim_y;
    const int tiles_x = (dim_x + diffuse::kTX - 1) / diffuse::kTX, tile_y = blockIdx.x / tiles_x;   // (tiles of a row run fastest)
    t.x0 = (blockIdx.x - tile_y * tiles_x) * diffuse::kTX;
    t.y0 = tile_y * diffuse::kTY;
    t.k = k;
    t.a = a;
    t.c = c;
    t.zero_solids = zero_solids;
    diffuse::Cells cells;
    diffuse::load(cells, lds, t, threadIdx.x);
    __syncthreads();
    for (int it = 0; it < k; ++it) {   // colour 0 = even (i + j) first
        diffuse::half_sweep(cells, lds, 0, t, threadIdx.x);
        __syncthreads();
        diffuse::half_sweep(cells, lds, 1, t, threadIdx.x);
        __syncthreads();
    }
    diffuse::store(lds, t, threadIdx.x);
}

}  // namespace

hipError_t launch_diffuse_velocity(hipStream_t s, float *u_out, const float *u_in, const float *u0, const uint8_t *codes,
                                   int dim_x, int dim_y, int k, float a, float c, bool zero_solids)
{
    if (k < 1 || k > diffuse::kD || u_out == u_in || u_out == u0 || dim_x < 1 || dim_y < 1) return hipErrorInvalidValue;
    const int64_t tiles = (int64_t)diffuse::tiles_x(dim_x) * diffuse::tiles_y(dim_y);   // one workgroup each, in one dimension
    if (tiles > INT32_MAX) return hipErrorInvalidValue;   // (a context holds 2^28 cells at most: 2^17 tiles and a ragged rim)
    diffuse_kernel<<<(unsigned)tiles, diffuse::kThreads, 0, s>>>(reinterpret_cast<diffuse::Vec2 *>(u_out),
                                                                  reinterpret_cast<const diffuse::Vec2 *>(u_in),
                                                                  reinterpret_cast<const diffuse::Vec2 *>(u0), codes, dim_x, dim_y, k, a, c,
                                                                  zero_solids);
    return hipGetLastError();
}

}  // namespace sfl
