// orb_pattern.h — the test pattern of rotated BRIEF for every orb_wta_k / orb_patch_size, host-pure: OpenCV 3's RNG (a 64-bit
// multiply-with-carry generator), makeRandomPattern (the 512-point pool of every patch size other than 31), initializeOrbPattern (the
// tuples of WTA_K 3 / 4 drawn from the pool) and the geometry that goes with a patch size (half patch, umax of ICAngles, the reach of
// the rotated points).  No HIP types and no library state: orb_kernels.hip takes its patterns from here and
// tests/cpp/orb_pattern_host_main.cpp compiles this file with the host compiler and writes every pattern out for the numpy statement
// (tests/np_orb_wta.py) to compare.  Restated from the published algorithm (features2d/src/orb.cpp, core's RNG); parity with OpenCV
// itself is unpinned, as for the rest of the front-end.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>

namespace stvo {

constexpr int ORB_POOL_POINTS = 512;     // points of the pool = int8 pairs of a 1024-byte pattern
constexpr int ORB_MAX_PATCH = 63;        // half patch 31: coordinates fit the int8 pattern, 89 x 89 blurred bytes per key-point
constexpr int ORB_MAX_HALF_PATCH = ORB_MAX_PATCH / 2;

// verdicts of the generator (the C-ABI maps them to STVO_OK / STVO_ERR_INVALID_ARG / STVO_ERR_UNSUPPORTED)
enum OrbPatternVerdict { ORB_PATTERN_OK = 0, ORB_PATTERN_INVALID = 1, ORB_PATTERN_UNSUPPORTED = 2 };

// cv::RNG: state = (uint32)state * 4164903690 + (state >> 32), the low word is the draw; a zero seed becomes 0xffffffff
struct OrbRng {
    uint64_t state;
    explicit OrbRng(uint64_t seed) : state(seed ? seed : 0xffffffffull) {}
    uint32_t next() {
        state = (uint64_t)(uint32_t)state * 4164903690ull + (state >> 32);
        return (uint32_t)state;
    }
    int uniform(int a, int b) { return a == b ? a : (int)(next() % (uint32_t)(b - a)) + a; }
};

// seeded stand-in for OpenCV's learned table of patch size 31 (data this repository does not hold: stvo_orb_set_pattern)
inline void orb_default_pool(int8_t* pattern /*[1024]*/) {
    uint32_t s = 31u;
    for (int i = 0; i < 256; ++i) {
        int v[4];
        do {
            for (int j = 0; j < 4; ++j) {
                s = s * 1664525u + 1013904223u;
                v[j] = (int)((s >> 16) % 27u) - 13;
            }
        } while (v[0] == v[2] && v[1] == v[3]);
        for (int j = 0; j < 4; ++j) pattern[4 * i + j] = (int8_t)v[j];
    }
}

// makeRandomPattern: 512 points, x then y, each uniform in [-P / 2, P / 2] (integer division)
inline void orb_random_pool(int patch_size, int8_t* pool /*[1024]*/) {
    OrbRng rng(0x34985739u);
    const int h = patch_size / 2;
    for (int i = 0; i < ORB_POOL_POINTS; ++i) {
        pool[2 * i] = (int8_t)rng.uniform(-h, h + 1);
        pool[2 * i + 1] = (int8_t)rng.uniform(-h, h + 1);
    }
}

inline int orb_pattern_points(int wta_k) { return wta_k == 2 ? 512 : 128 * wta_k; }

inline int orb_cv_ceil(double v) { return (int)std::ceil(v); }

// what a descriptor setting needs around a key-point: the half patch of the moments and the reach of the rotated pattern points.
// Patch 31 keeps the pool of +-13 (the learned table's range, stvo_orb_set_pattern) and with it the reach 19 the detector has always
// required; every other patch size draws points up to +-h, which a rotation takes to h sqrt 2
inline int orb_half_patch(int patch_size) { return patch_size / 2; }
inline int orb_reach(int patch_size) { return patch_size == 31 ? 19 : orb_cv_ceil(orb_half_patch(patch_size) * std::sqrt(2.0)); }

// umax of ICAngles for half patch h: u[v] = the half width of the disc's row |v|, v = 0 .. h (u[h + 1] is scratch of the symmetry pass)
inline void orb_umax(int h, int* u /*[h + 2]*/) {
    const int vmax = (int)std::floor(h * std::sqrt(2.0) / 2 + 1), vmin = (int)std::ceil(h * std::sqrt(2.0) / 2);
    for (int v = 0; v <= h + 1; ++v) u[v] = 0;
    for (int v = 0; v <= vmax; ++v) u[v] = (int)std::lrint(std::sqrt((double)h * h - (double)v * v));
    for (int v = h, v0 = 0; v >= vmin; --v) {
        while (u[v0] == u[v0 + 1]) ++v0;
        u[v] = v0;
        ++v0;
    }
}

// wta_k in {2, 3, 4}; patch_size 2 .. 63.  (The border rule needs a detector's edge threshold and is not judged here.)
inline int orb_descriptor_verdict(int wta_k, int patch_size) {
    if (wta_k < 2 || wta_k > 4 || patch_size < 2) return ORB_PATTERN_INVALID;
    if (patch_size > ORB_MAX_PATCH) return ORB_PATTERN_UNSUPPORTED;
    return ORB_PATTERN_OK;
}

// The effective point list of a setting in out[1024] (zero beyond 2 * n_points bytes).  pool31: the pool of patch size 31 (NULL: the
// stand-in); every entry must lie in -13 .. 13, and for WTA_K 3 / 4 it must hold at least wta_k different points (the draw below would
// not end otherwise).  It plays no part for any other patch size.
inline int orb_effective_pattern(int wta_k, int patch_size, const int8_t* pool31, int8_t* out /*[1024]*/, int* n_points) {
    const int verdict = orb_descriptor_verdict(wta_k, patch_size);
    if (verdict != ORB_PATTERN_OK) return verdict;
    int8_t pool[2 * ORB_POOL_POINTS];
    if (patch_size == 31) {
        if (pool31) {
            for (int i = 0; i < 2 * ORB_POOL_POINTS; ++i)
                if (pool31[i] < -13 || pool31[i] > 13) return ORB_PATTERN_INVALID;
            std::memcpy(pool, pool31, sizeof pool);
        } else {
            orb_default_pool(pool);
        }
    } else {
        orb_random_pool(patch_size, pool);
    }
    const int n = orb_pattern_points(wta_k);
    if (wta_k == 2) {
        std::memcpy(out, pool, sizeof pool);
        if (n_points) *n_points = n;
        return ORB_PATTERN_OK;
    }
    {   // different points in the pool: the first wta_k of them are enough to know that every tuple can be completed
        int distinct = 0;
        int8_t seen[4][2];
        for (int i = 0; i < ORB_POOL_POINTS && distinct < wta_k; ++i) {
            bool fresh = true;
            for (int j = 0; j < distinct; ++j) fresh = fresh && !(seen[j][0] == pool[2 * i] && seen[j][1] == pool[2 * i + 1]);
            if (fresh) {
                seen[distinct][0] = pool[2 * i];
                seen[distinct][1] = pool[2 * i + 1];
                ++distinct;
            }
        }
        if (distinct < wta_k) return ORB_PATTERN_INVALID;
    }
    int8_t eff[2 * ORB_POOL_POINTS];
    std::memset(eff, 0, sizeof eff);
    OrbRng rng(0x12345678u);
    for (int t = 0; t < 128; ++t)
        for (int k = 0; k < wta_k; ++k) {
            int8_t* tuple = eff + 2 * (t * wta_k);
            for (;;) {
                const int idx = rng.uniform(0, ORB_POOL_POINTS);
                const int8_t px = pool[2 * idx], py = pool[2 * idx + 1];
                int k1 = 0;
                while (k1 < k && !(tuple[2 * k1] == px && tuple[2 * k1 + 1] == py)) ++k1;
                if (k1 == k) {
                    tuple[2 * k] = px;
                    tuple[2 * k + 1] = py;
                    break;
                }
            }
        }
    std::memcpy(out, eff, sizeof eff);
    if (n_points) *n_points = n;
    return ORB_PATTERN_OK;
}

}  // namespace stvo
