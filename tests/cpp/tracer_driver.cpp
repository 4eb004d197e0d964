// tracer_driver.cpp -- TEST HARNESS.  Pathlines and probes by the per-point sample() every includer of "advect.h" sees
// (advect.h:24-72), from whichever "advect.h" the include path offers -- include/sfl or the reference's directory: a
// plain host program, no GPU.  For two shapes it fills the four fields of a step from a seeded LCG, places a set of
// tracers inside the domain, outside it on every side, on its corners and far away, advances them 6 times by the rule
// of include/sfl.h ("ADVANCE": u = sample(velocity, x, y, no_slip = true), then one rounded product and one rounded sum
// per component) and samples the four fields at the final positions with and without no_slip.  It prints bits only:
//
//     P <dim_x> <dim_y> <advance> <tracer> <x bits> <y bits>          advance 0 = the starts
//     S <dim_x> <dim_y> <no_slip> <tracer> <v.x> <v.y> <dye r g b> <pressure> <divergence>
//
// tests/test_tracers.py compares the build against include/sfl with tests/golden/tracers_reference.txt, written by
// tests/golden/make_tracer_goldens.py from the build against the reference.  Compiled with -DTRACER_DRIVER_FIELDS it also prints
// the fields and dt, which the generator turns into the .npz fixtures of the GPU tests:
//
//     D <dim_x> <dim_y> <dt bits> <tracers>
//     F <dim_x> <dim_y> <cell> <v.x> <v.y> <dye r g b> <pressure> <divergence>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "advect.h"
#include "uq32.h"

static uint32_t bits(float f)
{
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

static void run(int dim_x, int dim_y, int n, uint32_t seed, float dt, bool fields)
{
    const int cells = dim_x * dim_y;
    std::vector<Vector2<float>> v(cells);
    std::vector<Vector3<UQ32>> c(cells);
    std::vector<float> p(cells), d(cells);
    uint32_t s = seed;
    auto next = [&] { return s = s * 1664525u + 1013904223u; };
    auto real = [&](int span, float scale) { return float(int((next() >> 8) % (2 * span + 1)) - span) / scale; };
    for (int k = 0; k < cells; ++k) {
        v[k].x = real(1000, 100.0f);   // up to +-10 cells per unit of time: 3 cells per advance at dt = 0.3
        v[k].y = real(1000, 100.0f);
        c[k].x.raw = next() >> 1;
        c[k].y.raw = next() >> 1;
        c[k].z.raw = next() >> 1;
        p[k] = real(5000, 1000.0f);
        d[k] = real(5000, 1000.0f);
    }
    const float lx = float(dim_x - 1), ly = float(dim_y - 1), inf = HUGE_VALF;
    // the walls and corners from both sides of the half cell at which the no-slip weight reaches zero, the domain's own
    // corners, the last interior half cell, far away and infinitely far away
    const float special[][2] = {
        {-0.25f, 3.5f}, {-0.75f, 5.25f}, {lx + 0.25f, 2.5f}, {lx + 0.625f, 4.5f}, {3.5f, -0.25f}, {4.5f, -2.0f},
        {5.5f, ly + 0.375f}, {6.5f, ly + 1.0f}, {-0.125f, -0.375f}, {lx + 0.125f, -0.4375f}, {-0.3125f, ly + 0.25f},
        {lx + 0.2f, ly + 0.3f}, {-3.0f, -3.0f}, {0.0f, 0.0f}, {lx, ly}, {lx - 0.5f, 0.5f}, {-0.5f, 1.5f}, {1.5f, ly + 0.5f},
        {1e30f, 2.0f}, {-1e30f, 1e30f}, {inf, 1.25f}, {2.75f, -inf}, {-inf, inf}, {lx - 0.001f, ly - 0.001f}};
    const int n_special = int(sizeof special / sizeof special[0]);
    std::vector<float> x(n), y(n);
    for (int k = 0; k < n; ++k) {
        if (k < n_special) {
            x[k] = special[k][0];
            y[k] = special[k][1];
        } else {   // from 1.5 cells outside one wall to 1.5 cells outside the other, in steps of 1/64
            x[k] = float(int((next() >> 8) % uint32_t((dim_x + 2) * 64))) / 64.0f - 1.5f;
            y[k] = float(int((next() >> 8) % uint32_t((dim_y + 2) * 64))) / 64.0f - 1.5f;
        }
    }
    if (fields) {
        std::printf("D %d %d %08x %d\n", dim_x, dim_y, bits(dt), n);
        for (int k = 0; k < cells; ++k)
            std::printf("F %d %d %d %08x %08x %08x %08x %08x %08x %08x\n", dim_x, dim_y, k, bits(v[k].x), bits(v[k].y), c[k].x.raw,
                        c[k].y.raw, c[k].z.raw, bits(p[k]), bits(d[k]));
    }
    for (int step = 0; step <= 6; ++step) {
        if (step > 0)
            for (int k = 0; k < n; ++k) {
                const Vector2<float> u = sample(v.data(), x[k], y[k], dim_x, dim_y, true);
                const float move_x = u.x * dt, move_y = u.y * dt;
                x[k] = x[k] + move_x;
                y[k] = y[k] + move_y;
            }
        for (int k = 0; k < n; ++k) std::printf("P %d %d %d %d %08x %08x\n", dim_x, dim_y, step, k, bits(x[k]), bits(y[k]));
    }
    for (int no_slip = 0; no_slip < 2; ++no_slip)
        for (int k = 0; k < n; ++k) {
            const Vector2<float> a = sample(v.data(), x[k], y[k], dim_x, dim_y, no_slip != 0);
            const Vector3<UQ32> b = sample(c.data(), x[k], y[k], dim_x, dim_y, no_slip != 0);
            const float q = sample(p.data(), x[k], y[k], dim_x, dim_y, no_slip != 0);
            const float e = sample(d.data(), x[k], y[k], dim_x, dim_y, no_slip != 0);
            std::printf("S %d %d %d %d %08x %08x %08x %08x %08x %08x %08x\n", dim_x, dim_y, no_slip, k, bits(a.x), bits(a.y), b.x.raw,
                        b.y.raw, b.z.raw, bits(q), bits(e));
        }
}

int main()
{
#ifdef TRACER_DRIVER_FIELDS
    const bool fields = true;
#else
    const bool fields = false;
#endif
    run(33, 17, 97, 4711u, 0.3f, fields);
    run(61, 81, 161, 1234567u, 0.25f, fields);
    return 0;
}
