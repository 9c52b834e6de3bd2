// The product's csrc/lsd_scale_plan.h on the host, for tests/test_lsd_scale_plan_host.py — TEST INFRASTRUCTURE ONLY.
#include <cstdint>

#include "../../stvo-pl_amd/csrc/lsd_scale_plan.h"

extern "C" {

int lph_budget() { return stvo::BR_LDS_BUDGET; }

// the plan of one image size: out = tw_log, th_log, lds_bytes; 0 where no tile fits
int lph_plan(int cols, int rows, double scale, int radius, int32_t* out) {
    stvo::BlurResizePlan p{};
    if (!stvo::plan_blur_resize_u8(cols, rows, scale, radius, &p)) return 0;
    out[0] = p.tw_log; out[1] = p.th_log; out[2] = p.lds_bytes;
    return 1;
}

// br_layout, field by field: out = sr, scp, ncp; returns bytes
long long lph_layout(int nx, int ny, int ncp, int nr, int hk, int tw, int th, int32_t* out) {
    const stvo::BrLayout l = stvo::br_layout(nx, ny, ncp, nr, hk, tw, th);
    out[0] = l.sr; out[1] = l.scp; out[2] = l.ncp;
    return l.bytes;
}

// one tile: out = nx, xlist, ylist, nr, sr, scp, ncp; returns bytes
long long lph_tile(int cmin, int cmax, int rmin, int rmax, int ntw, int nth, int hk, int tw, int th, int32_t* out) {
    int nx = 0, nr = 0;
    bool xlist = false, ylist = false;
    const stvo::BrLayout l = stvo::br_tile_layout(cmin, cmax, rmin, rmax, ntw, nth, hk, tw, th, nx, xlist, ylist, nr);
    out[0] = nx; out[1] = xlist; out[2] = ylist; out[3] = nr; out[4] = l.sr; out[5] = l.scp; out[6] = l.ncp;
    return l.bytes;
}

// the largest need over every tile of an image: tile column i has the taps xc[i] = (cmin, cmax, ntw), tile row j has yr[j] = (rmin, rmax, nth)
long long lph_max_tile_bytes(int ntx, const int32_t* xc, int nty, const int32_t* yr, int hk, int tw, int th) {
    long long most = 0;
    for (int j = 0; j < nty; ++j)
        for (int i = 0; i < ntx; ++i) {
            int nx, nr;
            bool xlist, ylist;
            const long long b = stvo::br_tile_layout(xc[3 * i], xc[3 * i + 1], yr[3 * j], yr[3 * j + 1], xc[3 * i + 2], yr[3 * j + 2], hk, tw, th,
                                                     nx, xlist, ylist, nr).bytes;
            if (b > most) most = b;
        }
    return most;
}

}  // extern "C"
