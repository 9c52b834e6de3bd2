// The product's front-end layouts (stvo-pl_amd/csrc/frontend_layout.h) and gaussian_q8 (gaussian_q8.h) behind a flat C interface —
// TEST INFRASTRUCTURE ONLY.  Every layout runs on a base that is never dereferenced; an entry writes the offset of every buffer in the
// order the layout cuts them (-1: a conditional buffer that was not cut), then the total.  tests/frontend_layout_host_lib.py names the
// entries in the same order.  g++ alone builds it.  With FRONTEND_LAYOUT_HOST_MAIN it is a stand-alone program that walks a grid of
// geometries (the sanitizer build).
#include <cstdio>
#include <initializer_list>

#include "../../stvo-pl_amd/csrc/frontend_layout.h"
#include "../../stvo-pl_amd/csrc/gaussian_q8.h"

namespace {
// (a base other than null, so that a buffer at offset 0 and a buffer that was not cut differ)
char* const BASE = reinterpret_cast<char*>(uintptr_t(1) << 40);
long long at(const void* p) { return p ? (long long)(static_cast<const char*>(p) - BASE) : -1; }
int put(long long* out, std::initializer_list<const void*> ps, const stvo::Carver& c) {
    int n = 0;
    for (const void* p : ps) out[n++] = at(p);
    out[n++] = (long long)c.off;
    return n;
}
}  // namespace

extern "C" {

// what the Python side cannot know from include/: 0 .. 2 sizeof(LsdPx), sizeof(FldChain), sizeof(stvo_keyline); then LSD_UNIT, LSD_CTL,
// FLD_UNIT, FLD_BINS, FLD_SEG_CAP, LBD_DESC_FLOATS
int flh_const(int i) {
    const int v[] = {(int)sizeof(stvo::LsdPx), (int)sizeof(stvo::FldChain), (int)sizeof(stvo_keyline), stvo::LSD_UNIT, stvo::LSD_CTL,
                     stvo::FLD_UNIT,           stvo::FLD_BINS,              stvo::FLD_SEG_CAP,         stvo::LBD_DESC_FLOATS};
    return i >= 0 && i < (int)(sizeof v / sizeof v[0]) ? v[i] : -1;
}

// pattern, th_own, effective, then twelve entries per level, then the total
int flh_orb_arena(int B, int K, int nlevels, const int* cols, const int* rows, long long* out) {
    stvo::Carver c(BASE);
    const stvo::OrbArena a = stvo::carve_orb_arena(c, B, K, nlevels, cols, rows);
    int n = 0;
    for (const void* p : {(const void*)a.pattern, (const void*)a.th_own, (const void*)a.effective}) out[n++] = at(p);
    for (int l = 0; l < nlevels; ++l) {
        const stvo::OrbLevelBufs& q = a.lev[l];
        for (const void* p : {(const void*)q.blur, (const void*)q.hist, (const void*)q.cand, (const void*)q.hkey, (const void*)q.n_cand, (const void*)q.img,
                              (const void*)q.kp, (const void*)q.resp, (const void*)q.ang, (const void*)q.desc, (const void*)q.n, (const void*)q.n_tot})
            out[n++] = at(p);
    }
    out[n++] = (long long)c.off;
    return n;
}
int flh_orb_cand_cap(int cols, int rows) { return stvo::orb_cand_cap(cols, rows); }

int flh_orb_staging(int B, int cols, int rows, int K, long long* out) {
    stvo::Carver c(BASE);
    const stvo::OrbStaging s = stvo::carve_orb_staging(c, B, cols, rows, K);
    return put(out, {s.img, s.kp, s.resp, s.ang, s.oct, s.desc, s.n, s.n_total}, c);
}

int flh_lbd_arena(int B, int cols, int rows, long long* out) {
    stvo::Carver c(BASE);
    const stvo::LbdArena a = stvo::carve_lbd_arena(c, B, cols, rows);
    return put(out, {a.blur, a.dxy}, c);
}

int flh_lbd_staging(int B, int cols, int rows, int M, long long* out) {
    stvo::Carver c(BASE);
    const stvo::LbdStaging s = stvo::carve_lbd_staging(c, B, cols, rows, M);
    return put(out, {s.img, s.lines, s.n, s.desc, s.desc_f}, c);
}

int flh_lsd_arena(int B, int cols, int rows, int w, int h, int n_bins, int seg_cap, int K, int blur7, long long* out) {
    stvo::Carver c(BASE);
    const stvo::LsdArena a = stvo::carve_lsd_arena(c, B, cols, rows, w, h, n_bins, seg_cap, K, blur7 != 0);
    return put(out, {a.blur, a.scaled, a.img, a.px, a.k32, a.cnt, a.order, a.reg, a.kmax, a.seg, a.n_seg, a.lines, a.response, a.n_lines, a.n_pass}, c);
}

int flh_lsd_xcd_route(int refine, int B, long long npx) { return stvo::lsd_xcd_route(refine, B, (size_t)npx) ? 1 : 0; }

// stamp, wlist, pend, ctl (inside pend's cut), the total, then the two spans a call clears
int flh_lsd_xcd_arena(int B, long long npx, int nw, long long* out) {
    stvo::Carver c(BASE);
    const stvo::LsdXcdArena a = stvo::carve_lsd_xcd_arena(c, B, (size_t)npx, (size_t)nw);
    int n = put(out, {a.stamp, a.wlist, a.pend, a.ctl}, c);
    out[n++] = (long long)a.stamp_bytes;
    out[n++] = (long long)a.pend_ctl_bytes;
    return n;
}

int flh_fld_arena(int B, int cols, int rows, int L, int K, long long* out) {
    stvo::Carver c(BASE);
    const stvo::FldArena a = stvo::carve_fld_arena(c, B, cols, rows, L, K);
    return put(out, {a.img, a.ebits, a.sbits, a.wsum, a.lab, a.tmp, a.list, a.cnt, a.n_edge, a.pts, a.ch_at, a.ch, a.n_ch, a.sg, a.dseg, a.n_seg, a.err,
                     a.lines, a.response, a.n_lines}, c);
}
// nw, nunits, the capacity of the chain and segment stores
void flh_fld_geometry(int npx, int L, int* out) {
    out[0] = stvo::fld_words(npx); out[1] = stvo::fld_units(npx); out[2] = stvo::fld_store_cap(npx, L);
}

int flh_rectify_staging(int B, int cols, int rows, long long* out) {
    stvo::Carver c(BASE);
    const stvo::StereoStaging s = stvo::carve_rectify_staging(c, B, cols, rows);
    return put(out, {s.src_l, s.src_r, s.dst_l, s.dst_r}, c);
}

int flh_color_rectify_staging(int n, int cols, int rows, int channels, long long* out) {
    stvo::Carver c(BASE);
    const stvo::StereoStaging s = stvo::carve_color_rectify_staging(c, n, cols, rows, channels);
    return put(out, {s.src_l, s.src_r, s.dst_l, s.dst_r}, c);
}

int flh_gray_staging(long long npix, int channels, long long* out) {
    stvo::Carver c(BASE);
    const stvo::GrayStaging s = stvo::carve_gray_staging(c, (size_t)npix, channels);
    return put(out, {s.src, s.gray, s.swapped}, c);
}

void flh_gaussian_q8(int radius, double sigma, int32_t* w) { stvo::gaussian_q8(radius, sigma, w); }
}

#ifdef FRONTEND_LAYOUT_HOST_MAIN
#include <cmath>

namespace {
int g_bad = 0, g_runs = 0;
// the offsets an entry wrote are multiples of 256 (or -1), ascending, and below the total at out[n_buf]
void check(const char* what, const long long* out, int n_buf) {
    long long prev = -1;
    for (int i = 0; i < n_buf; ++i) {
        if (out[i] < 0) continue;
        if (out[i] % 256 || out[i] <= prev || out[i] >= out[n_buf]) {
            std::printf("layout inconsistent: %s entry %d\n", what, i);
            ++g_bad;
        }
        prev = out[i];
    }
    ++g_runs;
}
}  // namespace

int main() {
    static long long out[128];
    for (int B : {1, 9})
        for (int nlevels : {1, 2, 8})
            for (int K : {1, 4096})
                for (int size : {64, 97, 4095}) {
                    int cols[STVO_ORB_MAX_LEVELS], rows[STVO_ORB_MAX_LEVELS];
                    for (int l = 0; l < nlevels; ++l) {
                        const float s = l ? (float)std::pow(1.2, (double)l) : 1.f;
                        cols[l] = l ? (int)std::lrintf((float)size / s) : size;
                        rows[l] = cols[l];
                    }
                    check("orb arena", out, flh_orb_arena(B, K, nlevels, cols, rows, out) - 1);
                    check("orb staging", out, flh_orb_staging(B, size, size, K, out) - 1);
                    check("lbd arena", out, flh_lbd_arena(B, size, size, out) - 1);
                    check("lbd staging", out, flh_lbd_staging(B, size, size, K, out) - 1);
                }
    for (int B : {1, 2, 128, 129})
        for (int n_bins : {1, 1024, 2048})
            for (int blur7 : {0, 1})
                for (const auto& wh : {std::initializer_list<int>{64, 48, 64, 48}, {64, 48, 51, 38}, {97, 61, 24, 15}, {1024, 768, 1024, 768}, {1024, 769, 1024, 769}}) {
                    const int* g = wh.begin();
                    check("lsd arena", out, flh_lsd_arena(B, g[0], g[1], g[2], g[3], n_bins, 8192, 300, blur7, out) - 1);
                    if (B <= 128) {  // (ctl lies inside pend's cut: three cuts, then the total)
                        (void)flh_lsd_xcd_arena(B, (long long)g[2] * g[3], B == 1 ? 65 : 5, out);
                        out[3] = out[4];
                        check("lsd xcd arena", out, 3);
                    }
                }
    for (int B : {1, 9})
        for (int L : {1, 5, 100000})
            for (int size : {16, 97, 1024}) check("fld arena", out, flh_fld_arena(B, size, size, L, 300, out) - 1);
    for (int B : {1, 9})
        for (int ch : {3, 4})
            for (int size : {16, 97, 1024}) {
                (void)flh_rectify_staging(B, size, size - 1, out);  // (one cut of four unpadded sides, then the total)
                out[1] = out[4];
                check("rectify staging", out, 1);
                check("colour rectify staging", out, flh_color_rectify_staging(B, size, size - 1, ch, out) - 1);
                check("grey staging", out, flh_gray_staging((long long)B * size * (size - 1), ch, out) - 1);
            }
    int32_t w[31];
    long long sum = 0;
    const double pairs[][2] = {{0, 0.0}, {1, 0.26}, {2, 1.0}, {3, 2.0}, {3, 0.75}, {4, 0.92}, {9, 2.4}, {14, 3.64}, {15, 4.0}};
    for (const auto& p : pairs) {
        stvo::gaussian_q8((int)p[0], p[1], w);
        for (int i = 0; i <= 2 * (int)p[0]; ++i) sum += w[i];
    }
    std::printf("%d layouts, %d inconsistent, weights sum %lld\n", g_runs, g_bad, sum);
    return g_bad ? 1 : 0;
}
#endif
