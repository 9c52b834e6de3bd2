// snapshot_host_main.cpp — TEST INFRASTRUCTURE ONLY: a stand-alone program that runs the plain C++ pack / unpack of the product's
// stream_snapshot.h on seeded random rows, with every array sized exactly to one stream's rows — built with
// -fsanitize=address,undefined by tests/test_stream_snapshot_host.py, so that a read or write outside a section ends the program.
// Exit status 0: every case round-tripped.
#include <cstdio>

#include "snapshot_host.cpp"

int main() {
    const int caps[][2] = {{64, 64}, {128, 64}, {512, 64}, {2048, 512}};
    int bad = 0, cases = 0;
    for (const auto& c : caps) {
        const int K = c[0], M = c[1];
        const int ns[] = {0, 1, K - 1, K}, nls[] = {0, 1, M};
        for (int flags = 0; flags < 32; ++flags) {
            if (!snap::flags_legal(flags)) continue;
            for (int n : ns)
                for (int nl : nls) {
                    // the key-frame set's counts differ from the set's; the target is cut at the same, a larger and the smallest capacity that fits
                    const int kf_n = (n * 7 + 3) % (K + 1), kf_nl = (nl * 5 + 1) % (M + 1);
                    const int need_K = (((n > kf_n || !(flags & STVO_SNAP_KF_SETS)) ? n : kf_n) + 63) & ~63;
                    const int Kt[] = {K, 2 * K, need_K ? need_K : 64};
                    for (int kt : Kt) {
                        const int rc = snh_roundtrip(K, M, flags, n, nl, kf_n, kf_nl, kt, M, (unsigned)cases);
                        if (rc) std::printf("K %d M %d flags %d n %d nl %d -> K' %d: failed check %d\n", K, M, flags, n, nl, kt, rc);
                        bad += rc != 0;
                        ++cases;
                    }
                }
        }
    }
    std::printf("snapshot_host_main: %d cases, %d failures\n", cases, bad);
    return bad ? 1 : 0;
}
