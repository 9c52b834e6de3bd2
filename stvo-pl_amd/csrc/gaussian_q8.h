// gaussian_q8.h — the 8-bit fixed-point Gaussian weights of the 8-bit blurs (ORB: radius 3, sigma 2; LBD: radius 2, sigma 1; LSD: the
// radius and sigma of stvo_lsd_geometry).  Host-pure.
#pragma once

#include <cmath>
#include <cstdint>

namespace stvo {

// getGaussianKernel(1 + 2 radius, sigma) in 8-bit fixed point: w[i] = lrint((float)(k_i / sum) 256), k_i = exp(-(i - radius)^2 / 2 sigma^2),
// the sum taken in the order of i.  Radius 0 is the identity, 256, and evaluates no Gaussian (sigma may be 0 there).
inline void gaussian_q8(int radius, double sigma, int32_t* w) {
    if (radius == 0) {
        w[0] = 256;
        return;
    }
    const auto k = [&](int i) {
        const double x = i - radius;
        return std::exp(-x * x / (2.0 * sigma * sigma));
    };
    double sum = 0.0;
    for (int i = 0; i <= 2 * radius; ++i) sum += k(i);
    for (int i = 0; i <= 2 * radius; ++i) w[i] = (int32_t)std::lrint((float)(k(i) / sum) * 256.0);
}

}  // namespace stvo
