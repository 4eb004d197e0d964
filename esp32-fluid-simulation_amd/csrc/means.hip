// means.hip -- the per-cell sums over time (gfx950 / MI355X; include/sfl.h "AVERAGES"): ONE launch adds the fields held to
// the planes of a whole-domain context of any size or of all recorded members of a batch.
//
// The rule is one rounded IEEE-754 double addition per plane and cell (one 64-bit integer addition for the dye), so there is
// nothing to reduce and nothing to order: a streaming read-modify-write, bound by memory -- 8 B of velocity, 4 B of pressure
// and 12 B of dye read per cell as far as the mask asks for them, 8 B read and 8 B written per live plane.  No atomics, no
// LDS, no scratch.
//   * a lane takes kMeanLaneCells = 2 neighbouring cells of one member: 16 bytes of velocity, 8 of pressure, 24 of dye, and
//     16 bytes -- one global_load_dwordx4, one global_store_dwordx4 -- of every plane;
//   * the PLANES are laid out for that (mean_kernels.h): a member's plane starts on 16 bytes because its stride is the
//     member's cells rounded up to an even number.  The value behind an odd member's last cell belongs to no cell: it
//     starts at zero, +0.0 (0) is added to it with every sample and it is never downloaded;
//   * the FIELDS are where the step left them: a member's velocity base is only 8-byte aligned and its dye base runs through
//     all four 4-byte alignments.  The loads ask for the alignment of a word only, as field_distance.hip's do (a
//     global_load_dwordx4 needs no more on this hardware), so there is no head to peel;
//   * the one cell behind the last whole lane of a member of odd size is read word by word by the lane that holds it (the
//     compiler folds that into the common path: it loads a lane's fields as one piece per cell, the second under the lane's
//     own condition -- the planes, four fifths of the bytes and more, move 16 bytes at a time);
//   * gridDim.x covers the lanes of one member (2^27 of them for 2^28 cells: 2^19 workgroups), gridDim.y the members, which a
//     workgroup strides over; every address is formed in 64 bits;
//   * the mask is uniform: its branches cost a scalar compare.
//
// Numerics: float -> double is exact, denormals included; the product of two floats is exact in a double, so that
// contraction could not change a bit (the unit is built with -ffp-contract=off all the same); NaN and +-Inf go the way IEEE
// sends them, into their own cell's sums.
#include "mean_kernels.h"

namespace sfl {
namespace {

typedef unsigned long long u64;

static_assert(kMeanLaneCells == 2, "the kernel below holds two cells per lane");

// N words that are read with one load of 4-byte alignment
template <int N>
struct __attribute__((packed, aligned(4))) Words {
    uint32_t w[N];
};

// two neighbouring values of a plane: at is even and the plane lies on 16 bytes
__device__ __forceinline__ void add2(double *__restrict__ plane, size_t at, double x0, double x1)
{
    double2 *q = reinterpret_cast<double2 *>(plane + at);
    double2 s = *q;
    s.x += x0;
    s.y += x1;
    *q = s;
}
__device__ __forceinline__ void add2(double *__restrict__ plane, size_t at, u64 x0, u64 x1)
{
    ulonglong2 *q = reinterpret_cast<ulonglong2 *>(plane + at);
    ulonglong2 s = *q;
    s.x += x0;
    s.y += x1;
    *q = s;
}

__global__ void __launch_bounds__(kMeanThreads) mean_sample_kernel(MeanSample a)
{
    const size_t c = ((size_t)blockIdx.x * kMeanThreads + threadIdx.x) * kMeanLaneCells;
    if (c >= a.cells) return;
    const bool two = c + 1 < a.cells;   // (false in one lane of a member of odd size)
    for (int m = blockIdx.y; m < a.count; m += gridDim.y) {   // workgroup-uniform
        const size_t cell = (size_t)(a.first + m) * a.cells + c, at = (size_t)m * a.member_stride + c;
        if (a.what & (SFL_MEAN_VELOCITY | SFL_MEAN_STRESS)) {
            const uint32_t *src = reinterpret_cast<const uint32_t *>(a.v) + cell * 2;
            Words<4> x;
            if (two) {
                x = *reinterpret_cast<const Words<4> *>(src);
            } else {   // the value behind the member's last cell takes +0.0
                x.w[0] = src[0], x.w[1] = src[1];
                x.w[2] = x.w[3] = 0u;
            }
            const double u0 = (double)__uint_as_float(x.w[0]), v0 = (double)__uint_as_float(x.w[1]);
            const double u1 = (double)__uint_as_float(x.w[2]), v1 = (double)__uint_as_float(x.w[3]);
            if (a.what & SFL_MEAN_VELOCITY) {
                add2(a.plane[SFL_MEAN_PLANE_U], at, u0, u1);
                add2(a.plane[SFL_MEAN_PLANE_V], at, v0, v1);
            }
            if (a.what & SFL_MEAN_STRESS) {
                add2(a.plane[SFL_MEAN_PLANE_UU], at, u0 * u0, u1 * u1);
                add2(a.plane[SFL_MEAN_PLANE_VV], at, v0 * v0, v1 * v1);
                add2(a.plane[SFL_MEAN_PLANE_UV], at, u0 * v0, u1 * v1);
            }
        }
        if (a.what & SFL_MEAN_PRESSURE) {
            const uint32_t *src = reinterpret_cast<const uint32_t *>(a.p) + cell;
            Words<2> x;
            if (two) {
                x = *reinterpret_cast<const Words<2> *>(src);
            } else {
                x.w[0] = src[0];
                x.w[1] = 0u;
            }
            const double p0 = (double)__uint_as_float(x.w[0]), p1 = (double)__uint_as_float(x.w[1]);
            add2(a.plane[SFL_MEAN_PLANE_P], at, p0, p1);
            add2(a.plane[SFL_MEAN_PLANE_PP], at, p0 * p0, p1 * p1);
        }
        if (a.what & SFL_MEAN_DYE) {
            const uint32_t *src = a.dye + cell * 3;
            Words<6> x;
            if (two) {
                x = *reinterpret_cast<const Words<6> *>(src);
            } else {
                x.w[0] = src[0], x.w[1] = src[1], x.w[2] = src[2];
                x.w[3] = x.w[4] = x.w[5] = 0u;
            }
            add2(a.plane[SFL_MEAN_PLANE_R], at, (u64)x.w[0], (u64)x.w[3]);
            add2(a.plane[SFL_MEAN_PLANE_G], at, (u64)x.w[1], (u64)x.w[4]);
            add2(a.plane[SFL_MEAN_PLANE_B], at, (u64)x.w[2], (u64)x.w[5]);
        }
    }
}

}  // namespace

hipError_t launch_mean_sample(hipStream_t s, const MeanSample &a)
{
    if (a.count < 1 || a.cells == 0 || !a.what) return hipSuccess;
    const size_t lanes = (a.cells + kMeanLaneCells - 1) / kMeanLaneCells;
    const dim3 grid((unsigned)((lanes + kMeanThreads - 1) / kMeanThreads), (unsigned)(a.count < kMeanMaxMemberBlocks ? a.count : kMeanMaxMemberBlocks));
    mean_sample_kernel<<<grid, kMeanThreads, 0, s>>>(a);
    return hipGetLastError();
}

}  // namespace sfl
