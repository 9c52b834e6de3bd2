// orb_rotate_host_main.cpp — TEST INFRASTRUCTURE ONLY: the product's csrc/orb_rotate.h compiled for the host, as a program of its own.
//   1. for float angles in [0, 360] degrees: orb_rotation's (a, b) against (float)cos((double)rad), (float)sin((double)rad) of the C
//      library, rad = angle * (float)(pi / 180) — bit for bit.  `full`: every float of the interval (1.13 G values); the default is
//      every 64th float plus 4 ulp to either side of every multiple of 45 degrees;
//   2. for every int8 pair in [-13, 13]^2 and every angle of a fixed list (the multiples of 45 degrees and their float neighbours, and
//      30 / 60-degree values whose products come close to halves): ORB_ROTATE_X / ORB_ROTATE_Y against the plain form round(x a - y b),
//      round(x b + y a) with every product and the sum rounded to float on its own (through exact doubles) and halves to even.
//      The same runs for every 4096th float angle of the interval.
// Exits non-zero at the first difference.  At most 16 threads.
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "../../stvo-pl_amd/csrc/orb_rotate.h"

static uint32_t bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}
static float from_bits(uint32_t u) {
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}

static std::atomic<int> g_bad{0};

static bool check_angle(float angle) {
    float a, b;
    stvo::orb_rotation(angle, a, b);
    const float rad = angle * (float)(3.14159265358979323846 / 180.0);
    const float ca = (float)std::cos((double)rad), sa = (float)std::sin((double)rad);
    if (bits(a) == bits(ca) && bits(b) == bits(sa)) return true;
    if (g_bad.fetch_add(1) == 0)
        std::fprintf(stderr, "angle %.9g (0x%08x): header (%.9g, %.9g), library (%.9g, %.9g)\n", (double)angle, bits(angle), (double)a, (double)b,
                     (double)ca, (double)sa);
    return false;
}

static bool check_points(float angle) {
    float a, b;
    stvo::orb_rotation(angle, a, b);
    for (int y = -13; y <= 13; ++y)
        for (int x = -13; x <= 13; ++x) {
            const float px = (float)(int8_t)x, py = (float)(int8_t)y;
            const int ix = ORB_ROTATE_X(px, py, a, b), iy = ORB_ROTATE_Y(px, py, a, b);
            // the plain form through doubles: a product of two floats is exact in double, so is the sum of two such products here
            // (|values| <= 26, cosines of float angles no smaller than 4e-8): one rounding to float each, as the float operations give
            const float xa = (float)((double)px * (double)a), yb = (float)((double)py * (double)b);
            const float xb = (float)((double)px * (double)b), ya = (float)((double)py * (double)a);
            const float sx = (float)((double)xa - (double)yb), sy = (float)((double)xb + (double)ya);
            const int rx = (int)std::nearbyint((double)sx), ry = (int)std::nearbyint((double)sy);   // halves to even (default mode)
            if (ix != rx || iy != ry) {
                if (g_bad.fetch_add(1) == 0) std::fprintf(stderr, "angle %.9g point (%d, %d): header (%d, %d), plain (%d, %d)\n", (double)angle, x, y, ix, iy, rx, ry);
                return false;
            }
        }
    return true;
}

int main(int argc, char** argv) {
    const bool full = argc > 1 && std::strcmp(argv[1], "full") == 0;
    const uint32_t hi = bits(360.0f), stride = full ? 1u : 64u;
    const int nthreads = 16;
    std::atomic<uint64_t> n_angles{0}, n_swept_points{0};
    std::vector<std::thread> pool;
    for (int t = 0; t < nthreads; ++t)
        pool.emplace_back([&, t] {   // non-negative floats are ordered as their words: thread t takes the words t, t + 16, ... of the stride
            uint64_t n = 0;
            for (uint64_t u = (uint64_t)t * stride; u <= hi && g_bad.load(std::memory_order_relaxed) == 0; u += (uint64_t)nthreads * stride) {
                check_angle(from_bits((uint32_t)u));
                ++n;
            }
            n_angles += n;
            n = 0;
            for (uint64_t u = (uint64_t)t * 4096u; u <= hi && g_bad.load(std::memory_order_relaxed) == 0; u += (uint64_t)nthreads * 4096u) {
                check_points(from_bits((uint32_t)u));   // every 4096th float angle: all 27 x 27 pattern points
                n += 27 * 27;
            }
            n_swept_points += n;
        });
    for (auto& th : pool) th.join();
    uint64_t n_near = 0, n_points = 0;
    std::vector<float> list;
    for (int k = 0; k <= 8; ++k) {
        const uint32_t c = bits(45.0f * (float)k);
        for (int d = -4; d <= 4; ++d) {
            if ((k == 0 && d < 0) || (k == 8 && d > 0)) continue;   // stay inside [0, 360]
            const float v = from_bits(c + (uint32_t)d);
            check_angle(v);
            list.push_back(v);
            ++n_near;
        }
    }
    for (float v : {30.0f, 60.0f, 120.0f, 150.0f, 210.0f, 240.0f, 300.0f, 330.0f, 44.990456f, 135.00955f, 224.99045f, 315.00955f})
        for (int d = -2; d <= 2; ++d) list.push_back(from_bits(bits(v) + (uint32_t)d));
    for (float v : list) {
        if (g_bad.load()) break;
        check_points(v);
        n_points += 27 * 27;
    }
    const int bad = g_bad.load();
    std::printf("%s sweep: %llu angles + %llu near the multiples of 45 degrees, %llu rotated points: %d mismatches\n", full ? "full" : "strided",
                (unsigned long long)n_angles.load(), (unsigned long long)n_near, (unsigned long long)(n_points + n_swept_points.load()), bad);
    return bad ? 1 : 0;
}
