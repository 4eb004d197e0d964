// torque_face.h -- a wet face's part in the torque of its body (include/sfl.h "TORQUE"), written ONCE for every user: the
// batch sampler and the context sampler of torque.hip and a host program that runs it face by face
// (tests/cpp/torque_driver.cpp).  The doubled arms of a face about the body's pivot, the bit length L(), the shift s that
// keeps the sums inside 64 bits, and the signed product of an arm and a term.  Plain C++ between SFL_HD: integers only, no
// float anywhere.  The face's terms themselves -- trunc(p * 2^-exp2) from the float's bits -- are body_walk.h's term_of.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#ifndef SFL_HD
#define SFL_HD __host__ __device__ __forceinline__
#endif
#else
#ifndef SFL_HD
#define SFL_HD inline
#endif
#endif

namespace sfl {
namespace torque_face {

// L(x): the bit length of x, 0 for 0
SFL_HD int bit_length(uint32_t x)
{
    int n = 0;
    for (int step = 16; step > 0; step >>= 1)
        if (x >> (n + step)) n += step;
    return x ? n + 1 : 0;
}

// s = max(0, L(faces) + L(max_arm2) - 30): what both exponents of a body are raised by
SFL_HD int shift_of(uint32_t faces, uint32_t max_arm2)
{
    const int s = bit_length(faces) + bit_length(max_arm2) - 30;
    return s > 0 ? s : 0;
}

struct Arms {
    int32_t rx2, ry2;   // 2 * iS - pivot2[0], 2 * jS - pivot2[1]
};

// the arms of the face of FLUID cell (i, j) whose solid cell S lies opposite dir (the fluid cell lies 0 = W, 1 = E, 2 = S,
// 3 = N of the solid one): the wall is at node S.  |i|, |j| < 2^28 and |pivot2| <= 2^24: no overflow in int32.
SFL_HD Arms arms_of(int i, int j, int dir, int32_t px2, int32_t py2)
{
    const int is = i + (dir == 0) - (dir == 1), js = j + (dir == 2) - (dir == 3);
    return Arms{2 * is - px2, 2 * js - py2};
}

// max(|rx2|, |ry2|)
SFL_HD uint32_t longest(Arms a)
{
    const uint32_t x = (uint32_t)(a.rx2 < 0 ? -a.rx2 : a.rx2), y = (uint32_t)(a.ry2 < 0 ? -a.ry2 : a.ry2);
    return x > y ? x : y;
}

// what the face adds to mp from its pressure term tp: rx * Fy - ry * Fx with the load record's signs (pressure pushes the
// body away from the fluid: fx takes +tp for dir 0, -tp for dir 1; fy +tp for dir 2, -tp for dir 3)
SFL_HD int64_t pressure_moment(Arms a, int dir, int64_t tp)
{
    const int64_t arm = dir < 2 ? -(int64_t)a.ry2 : (int64_t)a.rx2;
    return (dir & 1) ? -(arm * tp) : arm * tp;
}

// what it adds to mf from its tangential term tf: the friction record's plain signs (fy takes v.y for dir 0 and 1, fx takes
// v.x for dir 2 and 3)
SFL_HD int64_t friction_moment(Arms a, int dir, int64_t tf) { return dir < 2 ? (int64_t)a.rx2 * tf : -((int64_t)a.ry2 * tf); }

}  // namespace torque_face
}  // namespace sfl
