// field_distance.hip -- how far two sets of fields are apart without downloading them (gfx950 / MI355X): per record the
// maxima of |a - b| over the velocity components, the pressure and the dye channels, the exact sums of the dye's, and the
// number of CELLS whose bits differ.  What struct sfl_field_distance, sfl_distance and sfl_batch_distance report
// (include/sfl.h).
//
// Every figure reduces with an operation that does not depend on the order of reduction -- maxima over the bit patterns
// of |a - b| as unsigned integers (flow_stats.hip's max_abs_bits: finite values and +inf order as floats do, any NaN
// wins), unsigned maxima, counts and 64-bit integer sums -- so the results are bit-reproducible whatever the tiling.
//
// The three passes are one kernel template, bound by memory (16, 8 and 24 B per cell over both operands, a handful of
// operations per cell):
//   * a lane holds WHOLE cells, so that a differing cell is counted once without a word of its neighbours: one vector load
//     of kDist*LaneCells cells per operand -- two velocity cells or four pressure cells in 16 bytes, one dye cell in 12;
//   * the loads ask for the alignment of the field's ELEMENT only (8 B for the velocity, 4 B for the pressure and the dye:
//     a global_load_dwordx4 / dwordx3 needs no more than dword alignment on this hardware), so a member's base may sit
//     anywhere its elements may, the two operands need not share an alignment and there is no head to peel; every load
//     of the wave is contiguous (1 KiB, or 768 B of dye);
//   * a workgroup issues the kDistItemLoads loads per lane of BOTH operands of an item in front of its arithmetic: 16
//     loads in flight per lane; rows of the item past the member's end are clamped onto its last whole lane and ignored;
//   * the cells behind the last whole lane (cells modulo kDist*LaneCells, at most three) are read word by word by the
//     first lanes of the member's first item;
//   * work is dealt in ITEMS of one member to at most kMaxBlocks workgroups, which stride over the rest (a context is a
//     batch of one member); a workgroup reduces what it holds -- by __shfl_xor in the wave, through LDS across the waves
//     -- and issues ONE atomic per word when the member it works for changes and when it ends.  The records are zeroed on
//     the stream in front of the kernels.  The second operand has its own base and member stride (0: one fixed member).
//
// Numerics contract: -ffp-contract=off; a - b is one float32 subtraction, denormals kept.
#include <algorithm>

#include "../../include/sfl.h"
#include "ensemble_kernels.h"

namespace sfl {
namespace {

static_assert(sizeof(DistanceRecord) == sizeof(struct sfl_field_distance), "the device record is the public one");

typedef unsigned long long u64;

constexpr int kWaves = kDistThreads / 64;
constexpr int kMaxBlocks = 2048;   // 256 CUs x 8 workgroups: every wave slot of the chip once

// N words that are read with one load of 4-byte alignment
template <int N>
struct __attribute__((packed, aligned(4))) Words {
    uint32_t w[N];
};

// what a lane has gathered for the member its workgroup holds
template <int W, bool DYE>
struct Gathered {
    unsigned mx[W];
    unsigned differ;
    u64 sum[DYE ? W : 1];
};

template <int W, bool DYE>
__device__ __forceinline__ void clear(Gathered<W, DYE> &g)
{
#pragma unroll
    for (int w = 0; w < W; ++w) g.mx[w] = 0u;
    g.differ = 0u;
#pragma unroll
    for (int w = 0; w < (DYE ? W : 1); ++w) g.sum[w] = 0;
}

// one cell of W words from each side into g
template <int W, bool DYE>
__device__ __forceinline__ void cell_distance(Gathered<W, DYE> &g, const uint32_t *a, const uint32_t *b)
{
    bool differs = false;
#pragma unroll
    for (int w = 0; w < W; ++w) {
        differs |= a[w] != b[w];
        unsigned d;
        if (DYE) {
            d = a[w] > b[w] ? a[w] - b[w] : b[w] - a[w];
            g.sum[w] += d;
        } else {
            d = __float_as_uint(__uint_as_float(a[w]) - __uint_as_float(b[w])) & 0x7fffffffu;   // the bits of |a - b|
        }
        g.mx[w] = d > g.mx[w] ? d : g.mx[w];
    }
    g.differ += differs ? 1u : 0u;
}

// the workgroup's figures into the record: one atomic per word
template <int W, bool DYE>
__device__ __forceinline__ void flush(Gathered<W, DYE> &g, unsigned (*wave_mx)[3], unsigned *wave_differ, u64 (*wave_sum)[3], int lane,
                                      int wave, unsigned *mx_out, unsigned *differ_out, u64 *sum_out)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int w = 0; w < W; ++w) {
            const unsigned t = __shfl_xor(g.mx[w], o);
            g.mx[w] = t > g.mx[w] ? t : g.mx[w];
            if (DYE) g.sum[w] += __shfl_xor(g.sum[w], o);
        }
        g.differ += __shfl_xor(g.differ, o);
    }
    if (lane == 0) {
#pragma unroll
        for (int w = 0; w < W; ++w) {
            wave_mx[wave][w] = g.mx[w];
            if (DYE) wave_sum[wave][w] = g.sum[w];
        }
        wave_differ[wave] = g.differ;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int v = 1; v < kWaves; ++v) {
#pragma unroll
            for (int w = 0; w < W; ++w) {
                g.mx[w] = wave_mx[v][w] > g.mx[w] ? wave_mx[v][w] : g.mx[w];
                if (DYE) g.sum[w] += wave_sum[v][w];
            }
            g.differ += wave_differ[v];
        }
#pragma unroll
        for (int w = 0; w < W; ++w) {
            atomicMax(mx_out + w, g.mx[w]);
            if (DYE) atomicAdd(sum_out + w, g.sum[w]);
        }
        atomicAdd(differ_out, g.differ);
    }
    __syncthreads();   // (the LDS words are written again for the next member)
    clear(g);
}

// W words per cell, LC cells per lane and load.  a / b: the fields of member 0 as words, a_stride / b_stride: words from
// one member to the next.  mx_off / differ_off / sum_off: where the figures go inside a record, in 32-bit words.
template <int W, int LC, bool DYE>
__global__ void __launch_bounds__(kDistThreads)
distance_kernel(const uint32_t *__restrict__ a, size_t a_stride, const uint32_t *__restrict__ b, size_t b_stride, size_t cells,
                int members, long long items_per_member, int mx_off, int differ_off, int sum_off, DistanceRecord *__restrict__ out)
{
    constexpr int N = W * LC;
    constexpr size_t kRowCells = (size_t)kDistThreads * LC, kItemCells = kRowCells * kDistItemLoads;
    __shared__ unsigned wave_mx[kWaves][3];
    __shared__ unsigned wave_differ[kWaves];
    __shared__ u64 wave_sum[kWaves][3];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long items = (long long)members * items_per_member;
    const size_t whole = cells - cells % LC;   // the cells that lie in whole lanes
    Gathered<W, DYE> g;
    clear(g);
    int held = -1;   // the member whose figures g holds
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {   // workgroup-uniform
        const int member = (int)(item / items_per_member);
        const long long sub = item - (long long)member * items_per_member;
        if (member != held) {
            if (held >= 0) {
                unsigned *rec = reinterpret_cast<unsigned *>(out + held);
                flush(g, wave_mx, wave_differ, wave_sum, lane, wave, rec + mx_off, rec + differ_off, reinterpret_cast<u64 *>(rec + sum_off));
            }
            held = member;
        }
        const uint32_t *am = a + (size_t)member * a_stride, *bm = b + (size_t)member * b_stride;
        if (whole) {   // (workgroup-uniform)
            const size_t c0 = (size_t)sub * kItemCells + (size_t)threadIdx.x * LC;
            Words<N> xa[kDistItemLoads], xb[kDistItemLoads];
            // every load of the item first; a row past the member's end is loaded from its last whole lane and not read
#pragma unroll
            for (int k = 0; k < kDistItemLoads; ++k) {
                const size_t c = min(c0 + k * kRowCells, whole - LC);
                xa[k] = *reinterpret_cast<const Words<N> *>(am + c * W);
                xb[k] = *reinterpret_cast<const Words<N> *>(bm + c * W);
            }
#pragma unroll
            for (int k = 0; k < kDistItemLoads; ++k)
                if (c0 + k * kRowCells < whole) {
#pragma unroll
                    for (int q = 0; q < LC; ++q) cell_distance<W, DYE>(g, xa[k].w + q * W, xb[k].w + q * W);
                }
        }
        if (LC > 1 && sub == 0 && whole + threadIdx.x < cells) {   // the cells behind the last whole lane, one per lane
            const size_t c = whole + threadIdx.x;
            uint32_t ta[W], tb[W];
#pragma unroll
            for (int w = 0; w < W; ++w) ta[w] = am[c * W + w], tb[w] = bm[c * W + w];
            cell_distance<W, DYE>(g, ta, tb);
        }
    }
    if (held >= 0) {
        unsigned *rec = reinterpret_cast<unsigned *>(out + held);
        flush(g, wave_mx, wave_differ, wave_sum, lane, wave, rec + mx_off, rec + differ_off, reinterpret_cast<u64 *>(rec + sum_off));
    }
}

template <int W, int LC, bool DYE>
hipError_t launch_pass(hipStream_t s, DistanceRecord *out, const void *a, size_t a_member_cells, const void *b, size_t b_member_cells,
                       size_t cells, int members, size_t mx_off, size_t differ_off, size_t sum_off)
{
    const size_t item_cells = (size_t)kDistThreads * LC * kDistItemLoads;
    const long long items_per_member = (long long)((cells + item_cells - 1) / item_cells);
    const int blocks = (int)std::min<long long>((long long)members * items_per_member, kMaxBlocks);
    distance_kernel<W, LC, DYE><<<blocks, kDistThreads, 0, s>>>(static_cast<const uint32_t *>(a), a_member_cells * W,
                                                                 static_cast<const uint32_t *>(b), b_member_cells * W, cells, members,
                                                                 items_per_member, (int)(mx_off / 4), (int)(differ_off / 4),
                                                                 (int)(sum_off / 4), out);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_field_distance(hipStream_t s, DistanceRecord *out, int what, const DistanceSide &a, const DistanceSide &b,
                                 size_t cells, int members)
{
    hipError_t e = hipMemsetAsync(out, 0, sizeof(DistanceRecord) * (size_t)members, s);
    if (e != hipSuccess) return e;
    if (what & SFL_DIST_VELOCITY) {
        e = launch_pass<2, kDistVelocityLaneCells, false>(s, out, a.v, a.member_cells, b.v, b.member_cells, cells, members,
                                                          offsetof(DistanceRecord, max_abs_dvx), offsetof(DistanceRecord, velocity_cells_differ),
                                                          offsetof(DistanceRecord, sum_abs_ddye));
        if (e != hipSuccess) return e;
    }
    if (what & SFL_DIST_DYE) {
        e = launch_pass<3, kDistDyeLaneCells, true>(s, out, a.dye, a.member_cells, b.dye, b.member_cells, cells, members,
                                                    offsetof(DistanceRecord, max_abs_ddye), offsetof(DistanceRecord, dye_cells_differ),
                                                    offsetof(DistanceRecord, sum_abs_ddye));
        if (e != hipSuccess) return e;
    }
    if (what & SFL_DIST_PRESSURE) {
        e = launch_pass<1, kDistPressureLaneCells, false>(s, out, a.p, a.member_cells, b.p, b.member_cells, cells, members,
                                                          offsetof(DistanceRecord, max_abs_dp), offsetof(DistanceRecord, pressure_cells_differ),
                                                          offsetof(DistanceRecord, sum_abs_ddye));
    }
    return e;
}

}  // namespace sfl
