// Prints what the host Config mirror holds for orb_score: after the defaults, after each preset, and after reading the file given
// as argv[1] — test infrastructure (tests/test_harris_host.py), compiled with stvo-pl_amd/host/config.cpp alone.
#include <cstdio>

#include "config.h"

int main(int argc, char** argv) {
    using StVO::Config;
    std::printf("default %d\n", Config::orbScore());
    Config::setKittiPreset();
    std::printf("kitti %d\n", Config::orbScore());
    Config::setEurocPreset();
    std::printf("euroc %d\n", Config::orbScore());
    if (argc > 1) {
        Config::loadFromFile(argv[1]);
        std::printf("file %d\n", Config::orbScore());
    }
    return 0;
}
