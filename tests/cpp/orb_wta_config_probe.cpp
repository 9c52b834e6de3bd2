// Prints what the host Config mirror holds for orb_wta_k and orb_patch_size: after the defaults, after each preset, and after reading
// the file given as argv[1] — test infrastructure (tests/test_orb_wta_host.py), compiled with stvo-pl_amd/host/config.cpp alone.
#include <cstdio>

#include "config.h"

int main(int argc, char** argv) {
    using StVO::Config;
    std::printf("default %d %d\n", Config::orbWtaK(), Config::orbPatchSize());
    Config::setKittiPreset();
    std::printf("kitti %d %d\n", Config::orbWtaK(), Config::orbPatchSize());
    Config::setEurocPreset();
    std::printf("euroc %d %d\n", Config::orbWtaK(), Config::orbPatchSize());
    if (argc > 1) {
        Config::loadFromFile(argv[1]);
        std::printf("file %d %d\n", Config::orbWtaK(), Config::orbPatchSize());
    }
    return 0;
}
