// context_solids.hip -- a whole-domain context with solid cells inside its grid (gfx950 / MI355X; include/sfl.h "SOLIDS OF A
// CONTEXT"): the divergence, the pressure solve, the gradient and the two maxima of the solids' rule (include/sfl.h
// "SOLIDS", items 3 - 6) on a grid of ANY size.  Kernels of their own: the context's plain kernels derive their walls from
// coordinates and keep their text and their instructions, and a context without a mask launches exactly what it
// launched before.
//
// One CODE BYTE per cell, formed on the host (solids.cpp solid_codes) and read from memory: bits 0..3 = W, E, S, N
// neighbour present (inside the domain and fluid), bit 4 = the cell is fluid, a solid cell's byte 0 (advect_math.h).
//
// THE SOLVE is the hot path: solid_sor_kernel, the tile of sor_solid_tile.h -- a workgroup of 1024 threads owns 64 x 32
// cells, loads the 96 x 64 window around them into LDS (24 576 B: p alone, the colours apart, three cells of a colour
// per thread), runs up to kD = 8 iterations there and stores the owned cells to the ping-pong partner.  A solve of
// `iters` iterations is ceil(iters / kD) launches; the host swaps p and p_alt (context_solids.cpp).  No atomics, no
// inline assembly.  (DESIGN.md 4.12 and profiles/context_solids.txt have the shapes that were timed.)
//
// THE STREAMING KERNELS are one thread per cell with plain global loads -- a cell's few neighbours come from L2 / the
// vector cache, the pass is bound by its compulsory traffic: the divergence (item 4; inside a step it also stores (0, 0)
// into solid cells' velocity, item 3), the gradient (item 6), the masked update norm and the masked maximum of
// |divergence|.  Their stencils are advect_math.h's (divergence_sum_solid, project_cell_solid), the norm's relaxation
// sor_solid_tile.h's; the maxima are reduced as update_norm.hip reduces: bit patterns, wave by __shfl_xor, workgroup
// through LDS, one atomicMax per workgroup on a word zeroed on the stream in front -- any NaN wins.
//
// Numerics contract: -ffp-contract=off, every operation individually rounded in the rule's order.
#include <algorithm>

#include "advect_math.h"
#include "solid_kernels.h"
#include "sor_solid_tile.h"

namespace sfl {
namespace {

using namespace advect_math;

constexpr int kStreamThreads = 256, kStreamWaves = kStreamThreads / 64;
constexpr int kMaxBlocks = 2048;   // 256 CUs x 8 workgroups: what a reduction's grid is capped at (update_norm.hip)

// ---- the solve ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(solid_tile::kThreads)
solid_sor_kernel(float *__restrict__ p_out, const float *__restrict__ p_in, const float *__restrict__ d,
                 const uint8_t *__restrict__ codes, int dim_x, int dim_y, int k, SorParams prm)
{
    __shared__ float lds[solid_tile::kLdsFloats];
    solid_tile::Tile t;
    t.p_in = p_in;
    t.p_out = p_out;
    t.d = d;
    t.codes = codes;
    t.dim_x = dim_x;
    t.dim_y = dim_y;
    const int tiles_x = (dim_x + solid_tile::kTX - 1) / solid_tile::kTX, tile_y = blockIdx.x / tiles_x;   // (tiles of a row run fastest)
    t.x0 = (blockIdx.x - tile_y * tiles_x) * solid_tile::kTX;
    t.y0 = tile_y * solid_tile::kTY;
    t.k = k;
    t.dx = prm.dx;
    t.omega = prm.omega;
    t.one_minus_omega = prm.one_minus_omega;
    solid_tile::Cells c;
    solid_tile::load(c, lds, t, threadIdx.x);
    __syncthreads();
    for (int it = 0; it < k; ++it) {   // colour 0 = even (i + j) first
        solid_tile::half_sweep(c, lds, 0, t, threadIdx.x);
        __syncthreads();
        solid_tile::half_sweep(c, lds, 1, t, threadIdx.x);
        __syncthreads();
    }
    solid_tile::store(c, t, threadIdx.x);
}

// ---- one thread per cell -------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kStreamThreads)
solid_divergence_kernel(float *__restrict__ div, float *v, const uint8_t *__restrict__ codes, int dim_x, size_t cells,
                        float two_dx_inv, bool zero_solids)
{
    const size_t c = (size_t)blockIdx.x * kStreamThreads + threadIdx.x;
    if (c >= cells) return;
    const int code = codes[c];
    float2 *q = reinterpret_cast<float2 *>(v) + c;
    if (code & kSolidFluid) {
        div[c] = divergence_sum_solid(q, dim_x, code) * two_dx_inv;
    } else {   // (no fluid cell reads a solid cell's velocity: the store races with nothing)
        div[c] = 0.0f;
        if (zero_solids) *q = make_float2(0.0f, 0.0f);
    }
}

__global__ void __launch_bounds__(kStreamThreads)
solid_gradient_kernel(float *__restrict__ v, const float *__restrict__ p, const uint8_t *__restrict__ codes, int dim_x,
                      size_t cells, float two_dx_inv)
{
    const size_t c = (size_t)blockIdx.x * kStreamThreads + threadIdx.x;
    if (c >= cells) return;
    float2 *q = reinterpret_cast<float2 *>(v) + c;
    *q = project_cell_solid(*q, p + c, dim_x, codes[c], two_dx_inv);
}

// the workgroup's maximum of m into *worst (update_norm.hip's reduction)
__device__ __forceinline__ void reduce_max(unsigned m, unsigned *worst)
{
    __shared__ unsigned wave_worst[kStreamWaves];
    for (int o = 32; o > 0; o >>= 1) {   // the wave's maximum
        const unsigned t = __shfl_xor(m, o);
        m = t > m ? t : m;
    }
    if ((threadIdx.x & 63) == 0) wave_worst[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < kStreamWaves; ++k) m = wave_worst[k] > m ? wave_worst[k] : m;
        atomicMax(worst, m);
    }
}

__global__ void __launch_bounds__(kStreamThreads)
solid_update_norm_kernel(const float *__restrict__ p, const float *__restrict__ d, const uint8_t *__restrict__ codes, int dim_x,
                         size_t cells, float dx, unsigned *__restrict__ worst)
{
    unsigned m = 0u;
    for (size_t c = (size_t)blockIdx.x * kStreamThreads + threadIdx.x; c < cells; c += (size_t)gridDim.x * kStreamThreads) {
        const int code = codes[c];
        const int present = solid_tile::present_of(code);
        const float w = (code & kSolidW) ? p[c - 1] : -0.0f;
        const float e = (code & kSolidE) ? p[c + 1] : -0.0f;
        const float s = (code & kSolidS) ? p[c - dim_x] : -0.0f;
        const float n = (code & kSolidN) ? p[c + dim_x] : -0.0f;
        const float p_gs = solid_tile::gauss_seidel(dx * d[c], solid_tile::k_factor(present), solid_tile::z_term(present), w, e, s, n);
        const unsigned bits = __float_as_uint(p_gs - p[c]) & 0x7fffffffu;   // |p_gs - p|
        if (code & kSolidFluid) m = bits > m ? bits : m;   // (a solid cell has no say)
    }
    reduce_max(m, worst);
}

__global__ void __launch_bounds__(kStreamThreads)
solid_max_divergence_kernel(const float *__restrict__ v, const uint8_t *__restrict__ codes, int dim_x, size_t cells, float two_dx_inv,
                            unsigned *__restrict__ worst)
{
    unsigned m = 0u;
    const float2 *q = reinterpret_cast<const float2 *>(v);
    for (size_t c = (size_t)blockIdx.x * kStreamThreads + threadIdx.x; c < cells; c += (size_t)gridDim.x * kStreamThreads) {
        const int code = codes[c];
        const float sum = divergence_sum_solid(q + c, dim_x, code);
        const float dv = (code & kSolidFluid) ? sum * two_dx_inv : 0.0f;
        const unsigned bits = __float_as_uint(dv) & 0x7fffffffu;
        m = bits > m ? bits : m;
    }
    reduce_max(m, worst);
}

inline unsigned blocks_of(size_t cells) { return (unsigned)((cells + kStreamThreads - 1) / kStreamThreads); }
inline unsigned capped_blocks_of(size_t cells) { return std::min<unsigned>(blocks_of(cells), kMaxBlocks); }

}  // namespace

hipError_t launch_solid_divergence(hipStream_t s, float *div, float *v, const uint8_t *codes, int dim_x, int dim_y,
                                   float two_dx_inv, bool zero_solids)
{
    const size_t cells = (size_t)dim_x * (size_t)dim_y;
    if (cells == 0) return hipSuccess;
    solid_divergence_kernel<<<blocks_of(cells), kStreamThreads, 0, s>>>(div, v, codes, dim_x, cells, two_dx_inv, zero_solids);
    return hipGetLastError();
}

hipError_t launch_solid_gradient(hipStream_t s, float *v, const float *p, const uint8_t *codes, int dim_x, int dim_y,
                                 float two_dx_inv)
{
    const size_t cells = (size_t)dim_x * (size_t)dim_y;
    if (cells == 0) return hipSuccess;
    solid_gradient_kernel<<<blocks_of(cells), kStreamThreads, 0, s>>>(v, p, codes, dim_x, cells, two_dx_inv);
    return hipGetLastError();
}

hipError_t launch_solid_sor(hipStream_t s, float *p_out, const float *p_in, const float *d, const uint8_t *codes, int dim_x,
                            int dim_y, int k, SorParams prm)
{
    if (k < 1 || k > solid_tile::kD || p_out == p_in || dim_x < 1 || dim_y < 1) return hipErrorInvalidValue;
    const int64_t tiles = (int64_t)solid_tile::tiles_x(dim_x) * solid_tile::tiles_y(dim_y);   // one workgroup each, in one dimension
    if (tiles > INT32_MAX) return hipErrorInvalidValue;   // (a context holds 2^28 cells at most: 2^22 tiles and a ragged rim)
    solid_sor_kernel<<<(unsigned)tiles, solid_tile::kThreads, 0, s>>>(p_out, p_in, d, codes, dim_x, dim_y, k, prm);
    return hipGetLastError();
}

hipError_t launch_solid_update_norm(hipStream_t s, unsigned *worst, const float *p, const float *d, const uint8_t *codes,
                                    int dim_x, int dim_y, float dx)
{
    const size_t cells = (size_t)dim_x * (size_t)dim_y;
    hipError_t e = hipMemsetAsync(worst, 0, sizeof(unsigned), s);
    if (e != hipSuccess || cells == 0) return e;
    solid_update_norm_kernel<<<capped_blocks_of(cells), kStreamThreads, 0, s>>>(p, d, codes, dim_x, cells, dx, worst);
    return hipGetLastError();
}

hipError_t launch_solid_max_divergence(hipStream_t s, unsigned *worst, const float *v, const uint8_t *codes, int dim_x,
                                       int dim_y, float two_dx_inv)
{
    const size_t cells = (size_t)dim_x * (size_t)dim_y;
    hipError_t e = hipMemsetAsync(worst, 0, sizeof(unsigned), s);
    if (e != hipSuccess || cells == 0) return e;
    solid_max_divergence_kernel<<<capped_blocks_of(cells), kStreamThreads, 0, s>>>(v, codes, dim_x, cells, two_dx_inv, worst);
    return hipGetLastError();
}

}  // namespace sfl
