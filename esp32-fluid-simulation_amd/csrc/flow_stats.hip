// flow_stats.hip -- what a flow looks like without downloading it (gfx950 / MI355X): the maxima of |v.x|, |v.y| and
// |calculate_divergence(v, dx)| over a velocity field in one streaming pass, and the exact sum of every dye channel in one
// pass over the dye.  What struct sfl_flow_stats and sfl_batch_flow_stats[_each] report (include/sfl.h).
//
// Every figure reduces with an operation that does not depend on the order of reduction -- maxima over the bit patterns
// of |x| as unsigned integers (finite values and +inf order as floats do, any NaN wins, |-0.0f| is +0.0f) and 64-bit
// integer sums -- so the results are bit-reproducible whatever the tiling.  The divergence is advect_math.h's
// divergence_sum times 1 / (2 dx), the one statement of finitediff.cpp:9-39 every kernel of the library shares.
//
// Both passes are bound by memory (8 and 12 B per cell, a few operations per cell) and laid out as update_norm.hip's:
//   velocity  * a wave owns a TILE: a strip of 128 columns (64 lanes x one 16-byte load = two cells) and a chunk of rows
//               it walks down with the rows above and below in registers;
//             * W.x and E.x come from the lane's own two cells and from the neighbour lanes by DPP wave shifts; only
//               lane 0 and lane 63 load one more word per row, the x of the strip's outer neighbours; of the rows above
//               and below only y is used;
//             * row r + 2 and the outer words of row r + 1 are loaded in front of the arithmetic of row r;
//             * VEC = rows of 16-byte aligned cell pairs (dim_x even, aligned base): one global_load_dwordx4 per lane and
//               row.  Everything else takes two clamped 8-byte loads per lane: correct at any width and alignment.
//               Loads are unconditional and clamped into the field: what a clamped load returns never reaches a maximum.
//   dye       * the field is ONE stream of 3 * cells words; a wave takes it in blocks of 768 words = three 16-byte loads
//               per lane, each load of the wave contiguous.  768, 256 and 4 are 0, 1 and 1 modulo 3, so word j of load k
//               of lane l is channel (head + k + l + j) mod 3: the lane adds into three sums by COMPILE-TIME index and
//               rotates them once, at the end, by (head + l) mod 3;
//             * `head` = the words in front of the first 16-byte boundary (a batch member's base is aligned only when
//               its cell count is a multiple of 4); they and the words behind the last whole block are read one at a time;
//             * the loads of the wave's next block are issued in front of the sums of this one; sums are 64-bit: exact.
//   both      * work is dealt in ITEMS -- four tiles, or 32 dye blocks, of one member -- to at most kMaxBlocks
//               workgroups, which stride over the rest (a context is a batch of one member);
//             * a workgroup reduces what it holds -- by __shfl_xor in the wave, through LDS across the waves -- and issues
//               ONE atomic per word when the member it works for changes and when it ends: one per workgroup on a
//               context.  The records are zeroed on the stream in front of the kernels.
//
// Numerics contract: -ffp-contract=off, every operation individually rounded in the reference's order.
#include <algorithm>

#include "../../include/sfl.h"
#include "advect_math.h"
#include "stats_kernels.h"

namespace sfl {
namespace {

static_assert(sizeof(FlowStatsRecord) == sizeof(struct sfl_flow_stats), "the device record is the public one");

typedef float v4f __attribute__((ext_vector_type(4)));
typedef unsigned v4u __attribute__((ext_vector_type(4)));
typedef unsigned long long u64;

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kMaxBlocks = 2048;       // 256 CUs x 8 workgroups: every wave slot of the chip once
constexpr int kDyeBlockWords = 768;    // one wave: 64 lanes x three 16-byte loads
constexpr int kDyeItemBlocks = 32;     // dye blocks of one item: eight per wave

// DPP full-wave shifts (wave_shr:1 / wave_shl:1, as sor_lane.h): lane 0 / lane 63 receive 0 and take the strip's
// outer neighbour instead
__device__ __forceinline__ float lane_below(float x)  // value of lane - 1
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x138, 0xf, 0xf, false));
}
__device__ __forceinline__ float lane_above(float x)  // value of lane + 1
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x130, 0xf, 0xf, false));
}

// ---- the velocity pass --------------------------------------------------------------------------------------------
// the lane's two cells x, x + 1 of the row at `row` as {x.x, x.y, (x + 1).x, (x + 1).y}, columns clamped into the row
template <bool VEC>
__device__ __forceinline__ v4f load_cells(const float *row, int x, int dim_x)
{
    if (VEC) return *reinterpret_cast<const v4f *>(row + 2 * min(x, dim_x - 2));   // (dim_x is even: both in or both out)
    const float2 a = reinterpret_cast<const float2 *>(row)[min(x, dim_x - 1)];
    const float2 b = reinterpret_cast<const float2 *>(row)[min(x + 1, dim_x - 1)];
    return v4f{a.x, a.y, b.x, b.y};
}

// x of the strip's outer neighbours in one row: lane 0 gets cell x0 - 1, lane 63 cell x0 + 128 (where the field has them)
__device__ __forceinline__ float load_edge(const float *row, int lane, int x0, int dim_x)
{
    const int ex = lane == 0 ? x0 - 1 : x0 + kStatsStripCols;
    const bool has = (lane == 0 && x0 > 0) || (lane == 63 && ex < dim_x);
    return has ? row[2 * (size_t)ex] : 0.0f;
}

__device__ __forceinline__ unsigned max_abs_bits(unsigned m, float x)
{
    const unsigned bits = __float_as_uint(x) & 0x7fffffffu;   // |x|
    return bits > m ? bits : m;
}

// The lane's two cells of row r into the three running maxima.  s / n: the rows below / above (anything where the
// field has none: divergence_sum does not read them there), edge = load_edge of this row.
__device__ __forceinline__ void row_stats(unsigned (&m)[3], v4f s, v4f c, v4f n, float edge, int lane, int x, int r,
                                          int i_max, int j_max, float two_dx_inv)
{
    float west = lane_below(c.z), east = lane_above(c.x);
    west = lane == 0 ? edge : west;
    east = lane == 63 ? edge : east;
    const float wx[2] = {west, c.x}, ex[2] = {c.z, east};
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        // the cell's neighbourhood as divergence_sum addresses it: a 3 x 3 window, rows 3 apart, the cell in the middle
        // (of W and E it reads x, of S and N y; every index is a constant: the window lives in registers)
        float2 win[9] = {};
        win[4] = make_float2(c[2 * q], c[2 * q + 1]);
        win[3].x = wx[q];
        win[5].x = ex[q];
        win[1].y = s[2 * q + 1];
        win[7].y = n[2 * q + 1];
        const int i = x + q;
        const float d = advect_math::divergence_sum(win + 4, 3, i, r, i_max, j_max) * two_dx_inv;
        if (i <= i_max) {   // (a clamped column has no say)
            m[0] = max_abs_bits(m[0], win[4].x);
            m[1] = max_abs_bits(m[1], win[4].y);
            m[2] = max_abs_bits(m[2], d);
        }
    }
}

template <bool VEC>
__device__ __forceinline__ void velocity_tile(unsigned (&m)[3], const float *v, int dim_x, int dim_y, int strip, int chunk,
                                              int rows_per_tile, float two_dx_inv, int lane)
{
    const int j_max = dim_y - 1;
    const size_t pitch = 2 * (size_t)dim_x;   // floats per row
    const int x0 = strip * kStatsStripCols, x = x0 + 2 * lane;
    const int r0 = chunk * rows_per_tile, r1 = min(r0 + rows_per_tile, dim_y);
    // (loads are unconditional: a row the field does not have is loaded from the row beside it and never read)
    v4f below = load_cells<VEC>(v + (size_t)max(r0 - 1, 0) * pitch, x, dim_x);
    v4f cur = load_cells<VEC>(v + (size_t)r0 * pitch, x, dim_x);
    v4f above = load_cells<VEC>(v + (size_t)min(r0 + 1, j_max) * pitch, x, dim_x);
    float edge = load_edge(v + (size_t)r0 * pitch, lane, x0, dim_x);
    const int last_needed = min(r1, j_max);   // the row above the chunk's last, where the field has one
    for (int r = r0; r < r1; ++r) {
        // what row r + 1 needs first: its loads are in flight while row r is evaluated
        v4f next = above;
        float edge_next = edge;
        if (r + 1 < r1) {   // (wave-uniform)
            next = load_cells<VEC>(v + (size_t)min(r + 2, last_needed) * pitch, x, dim_x);
            edge_next = load_edge(v + (size_t)(r + 1) * pitch, lane, x0, dim_x);
        }
        row_stats(m, below, cur, above, edge, lane, x, r, dim_x - 1, j_max, two_dx_inv);
        below = cur;
        cur = above;
        above = next;
        edge = edge_next;
    }
}

// the workgroup's three maxima into the member's record: one atomicMax per word
__device__ __forceinline__ void flush_maxima(unsigned (&m)[3], unsigned (*wave_max)[3], int lane, int wave, FlowStatsRecord *rec)
{
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned t = __shfl_xor(m[k], o);
            m[k] = t > m[k] ? t : m[k];
        }
        if (lane == 0) wave_max[wave][k] = m[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int w = 1; w < kWaves; ++w) m[k] = wave_max[w][k] > m[k] ? wave_max[w][k] : m[k];
        atomicMax(&rec->max_abs_vx, m[0]);
        atomicMax(&rec->max_abs_vy, m[1]);
        atomicMax(&rec->max_abs_div, m[2]);
    }
    __syncthreads();   // (the LDS words are written again for the next member)
    m[0] = m[1] = m[2] = 0u;
}

template <bool VEC>
__global__ void __launch_bounds__(kThreads)
velocity_stats_kernel(const float *__restrict__ v, int dim_x, int dim_y, int members, int rows_per_tile, int strips, int tiles,
                      int items_per_member, float two_dx_inv, const float *__restrict__ member_two_dx_inv,
                      FlowStatsRecord *__restrict__ out)
{
    __shared__ unsigned wave_max[kWaves][3];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const size_t member_floats = 2 * (size_t)dim_x * (size_t)dim_y;
    const long long items = (long long)members * items_per_member;
    unsigned m[3] = {0u, 0u, 0u};
    int held = -1;   // the member whose maxima m holds
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {   // workgroup-uniform
        const int member = (int)(item / items_per_member), sub = (int)(item - (long long)member * items_per_member);
        if (member != held) {
            if (held >= 0) flush_maxima(m, wave_max, lane, wave, out + held);
            held = member;
        }
        const int tile = sub * kWaves + wave;   // wave-uniform
        if (tile < tiles) {
            const int chunk = tile / strips, strip = tile - chunk * strips;   // strips run fastest: neighbours in time share rows
            const float scale = member_two_dx_inv ? member_two_dx_inv[member] : two_dx_inv;
            velocity_tile<VEC>(m, v + (size_t)member * member_floats, dim_x, dim_y, strip, chunk, rows_per_tile, scale, lane);
        }
    }
    if (held >= 0) flush_maxima(m, wave_max, lane, wave, out + held);
}

// ---- the dye pass -------------------------------------------------------------------------------------------------
struct DyeBlock {
    v4u a[3];
};
// three 64-bit sums kept as three names, never indexed: they stay in registers
struct Sums {
    u64 a, b, c;
};

// block `b` of the aligned body: load k of the wave is 1 KiB contiguous
__device__ __forceinline__ DyeBlock load_block(const uint32_t *body, long long b, int lane)
{
    const v4u *q = reinterpret_cast<const v4u *>(body + b * kDyeBlockWords) + lane;
    return DyeBlock{{q[0], q[64], q[128]}};
}

// the workgroup's sums into the member's record: t = the lanes' sums by position in their loads (rotated here into
// channels, rot = (head + lane) mod 3), direct = sums by channel; one atomicAdd per channel
__device__ __forceinline__ void flush_sums(Sums &t, Sums &direct, int rot, u64 (*wave_sum)[3], int lane, int wave,
                                           FlowStatsRecord *rec)
{
    u64 s[3];
    s[0] = direct.a + (rot == 0 ? t.a : rot == 1 ? t.c : t.b);
    s[1] = direct.b + (rot == 0 ? t.b : rot == 1 ? t.a : t.c);
    s[2] = direct.c + (rot == 0 ? t.c : rot == 1 ? t.b : t.a);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s[k] += __shfl_xor(s[k], o);
        if (lane == 0) wave_sum[wave][k] = s[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
#pragma unroll
            for (int w = 1; w < kWaves; ++w) s[k] += wave_sum[w][k];
            atomicAdd(&rec->dye_sum[k], s[k]);
        }
    }
    __syncthreads();   // (the LDS words are written again for the next member)
    t = direct = Sums{0, 0, 0};
}

__global__ void __launch_bounds__(kThreads)
dye_stats_kernel(const uint32_t *__restrict__ dye, long long member_words, int members, int items_per_member,
                 FlowStatsRecord *__restrict__ out)
{
    __shared__ u64 wave_sum[kWaves][3];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long items = (long long)members * items_per_member;
    Sums t{0, 0, 0}, direct{0, 0, 0};   // by position in the lane's loads; by channel
    int held = -1, head = 0;   // the member whose sums t and direct hold, and the words in front of its aligned body
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {   // workgroup-uniform
        const int member = (int)(item / items_per_member), sub = (int)(item - (long long)member * items_per_member);
        const uint32_t *base = dye + (size_t)member * (size_t)member_words;
        if (member != held) {
            if (held >= 0) flush_sums(t, direct, (head + lane) % 3, wave_sum, lane, wave, out + held);
            held = member;
            head = (int)min((long long)((4u - (unsigned)(reinterpret_cast<uintptr_t>(base) >> 2)) & 3u), member_words);
        }
        const uint32_t *body = base + head;   // 16-byte aligned
        const long long blocks = (member_words - head) / kDyeBlockWords;
        const long long end = min(blocks, (long long)(sub + 1) * kDyeItemBlocks);
        long long b = (long long)sub * kDyeItemBlocks + wave;   // wave-uniform
        if (b < end) {
            DyeBlock cur = load_block(body, b, lane);
            for (; b < end; b += kWaves) {
                DyeBlock next = cur;   // the wave's next block first
                if (b + kWaves < end) next = load_block(body, b + kWaves, lane);
                // word j of load k into sum (k + j) mod 3
                t.a += cur.a[0].x, t.b += cur.a[0].y, t.c += cur.a[0].z, t.a += cur.a[0].w;
                t.b += cur.a[1].x, t.c += cur.a[1].y, t.a += cur.a[1].z, t.b += cur.a[1].w;
                t.c += cur.a[2].x, t.a += cur.a[2].y, t.b += cur.a[2].z, t.c += cur.a[2].w;
                cur = next;
            }
        }
        if (sub == 0) {   // the words in front of the body and behind its last whole block, one at a time
            const long long tail = head + blocks * kDyeBlockWords;
            const int loose = head + (int)(member_words - tail);
            for (int k = threadIdx.x; k < loose; k += kThreads) {
                const long long w = k < head ? k : tail + (k - head);
                const u64 value = base[w];
                const int c = (int)(w % 3);
                direct.a += c == 0 ? value : 0;
                direct.b += c == 1 ? value : 0;
                direct.c += c == 2 ? value : 0;
            }
        }
    }
    if (held >= 0) flush_sums(t, direct, (head + lane) % 3, wave_sum, lane, wave, out + held);
}

}  // namespace

hipError_t launch_flow_stats(hipStream_t s, FlowStatsRecord *out, int what, const float *v, const uint32_t *dye, int dim_x,
                             int dim_y, int members, float two_dx_inv, const float *member_two_dx_inv)
{
    hipError_t e = hipMemsetAsync(out, 0, sizeof(FlowStatsRecord) * (size_t)members, s);
    if (e != hipSuccess) return e;
    if (what & SFL_STATS_VELOCITY) {
        const int strips = (dim_x + kStatsStripCols - 1) / kStatsStripCols;
        // the tallest tile that still leaves every wave of the capped grid one (update_norm.hip: a taller tile re-reads
        // fewer rows, but tiles that do not fill the chip leave bandwidth idle); members of a batch count together
        int rows_per_tile = kStatsChunkRows;
        for (int r : {32, 16})
            if ((int64_t)members * strips * ((dim_y + r - 1) / r) >= (int64_t)kMaxBlocks * kWaves) {
                rows_per_tile = r;
                break;
            }
        const int tiles = strips * ((dim_y + rows_per_tile - 1) / rows_per_tile);
        const int items_per_member = (tiles + kWaves - 1) / kWaves;
        const int blocks = (int)std::min<int64_t>((int64_t)members * items_per_member, kMaxBlocks);
        const bool vec = dim_x % 2 == 0 && reinterpret_cast<uintptr_t>(v) % 16 == 0;
        if (vec)
            velocity_stats_kernel<true><<<blocks, kThreads, 0, s>>>(v, dim_x, dim_y, members, rows_per_tile, strips, tiles,
                                                                    items_per_member, two_dx_inv, member_two_dx_inv, out);
        else
            velocity_stats_kernel<false><<<blocks, kThreads, 0, s>>>(v, dim_x, dim_y, members, rows_per_tile, strips, tiles,
                                                                     items_per_member, two_dx_inv, member_two_dx_inv, out);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (what & SFL_STATS_DYE) {
        const long long member_words = 3ll * dim_x * dim_y;
        const int items_per_member = (int)std::max<long long>(1, (member_words / kDyeBlockWords + kDyeItemBlocks - 1) / kDyeItemBlocks);
        const int blocks = (int)std::min<int64_t>((int64_t)members * items_per_member, kMaxBlocks);
        dye_stats_kernel<<<blocks, kThreads, 0, s>>>(dye, member_words, members, items_per_member, out);
        e = hipGetLastError();
    }
    return e;
}

}  // namespace sfl
