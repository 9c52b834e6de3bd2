// lsd_scale_plan.h — the LDS geometry of lsd_blur_resize_kernel (lsd_scale_kernels.hip), host-pure (no HIP): the layout of one tile, the
// same arithmetic on the host (an upper bound sizes the launch) and in the kernel, and the plan of a launch (tile of the scaled image,
// dynamic LDS) for one image size.  tests/test_lsd_scale_plan_host.py runs this header on the host (tests/cpp/lsd_scale_plan_host.cpp).
//
// THE BOUND under a size table (stvo_lsd_set_image_sizes; the MIXED instance of the kernel runs every image under the SLOT's plan):
// for cols_i <= cols and rows_i <= rows, every tile of image i under the slot's tile fits the slot's lds_bytes.
//   - br_layout grows with each of nx, ny, ncp, nr (every term is a sum or a product of them with non-negative factors).
//   - plan_blur_resize_u8 takes for the slot  nx = min(window_x, cols), ny = min(window_y, rows),  ncp = min(run(nx), max(2 tw, 4)),
//     nr = min(ny, 2 th),  window = ceil((tile - 1) / scale) + 4: what the taps of a full tile can span at most, whatever the image.
//   - a tile of image i spans  nx_i <= min(window_x, cols_i) <= nx  columns (its taps lie inside its own cols_i, and a clipped tile spans
//     no more than a full one), likewise  ny_i <= ny;  br_tile_layout keeps  ncp_i = run(nx_i) only where nx_i <= 2 ntw <= 2 tw, else
//     2 ntw rounded up to 4 <= max(2 tw, 4): ncp_i <= ncp;  nr_i = ny_i where ny_i <= 2 nth, else 2 nth: nr_i <= nr.
//   So the image's need is the slot's formula at arguments that are each no larger.  Every size lsd_image_size_ok accepts also has a
// plan of its own (the loop below ends at a tile the smaller size fits no later than the slot), and the kernel's result does not depend
// on the tile: integer arithmetic per output pixel.
#pragma once

#if defined(__HIPCC__)
#define STVO_BR_HD __host__ __device__
#else
#define STVO_BR_HD
#endif

#include <cmath>

namespace stvo {

constexpr int BR_LDS_BUDGET = 64 * 1024;  // dynamic LDS a tile may take (no opt-in needed; the default 64 x 16 tile takes 34 KB at h = 5 / scale 0.5)

struct BlurResizePlan {
    int tw_log, th_log, lds_bytes;
};

// The geometry of a tile in LDS, the same arithmetic on the host (an upper bound sizes the launch) and in the kernel.  nx x ny: the
// source pixels between the tile's first and last bilinear tap; ncp x nr: the columns / rows in which blurred bytes are kept.
struct BrLayout {
    int sr;         // staged rows: ny + 2 radius
    int scp;        // pitch of a staged row in bytes: the columns a run of 4 sums reads (4 ceil(nx / 4) + 2 radius, in whole words)
    int ncp;        // pitch of the sums and of the blurred bytes, a multiple of 4: nx columns for a contiguous run, 2 per output column for the pairs
    long long bytes;
};
STVO_BR_HD inline BrLayout br_layout(int nx, int ny, int ncp, int nr, int hk, int tw, int th) {
    BrLayout l;
    l.sr = ny + 2 * hk;
    l.scp = (4 * ((nx + 3) / 4) + 2 * hk + 4) & ~3;
    l.ncp = ncp;
    l.bytes = 4ll * l.sr * ncp + 16 * (tw + th) + (long long)l.sr * l.scp + (((long long)nr * ncp + 3) & ~3ll);
    return l;
}

// One tile of one image: ntw x nth outputs (the tile clipped to the image's scaled size) whose first and last bilinear taps are the
// source columns cmin .. cmax and rows rmin .. rmax.  The taps are kept as one contiguous run, or — where they span more than 2 x the
// tile (scale < 0.5) — as the list of pairs per output.
// Out: nx (source columns between the first and the last tap), xlist / ylist (the taps as pairs per output, not as one contiguous run),
// nr (rows in which blurred bytes are kept) and the layout.
// The kernel keeps these four lines as its own text rather than calling this function: with the call (in this form, as a returned
// struct, or force-inlined) the radius-2 uniform instance came out of the compiler with another scalar register allocation, and the
// uniform instances are to stay the code they were (profiles/mixed_lsd_scale_kernel_resources.txt).  The two texts are the same
// statements — the four lines below and the four in lsd_scale_kernels.hip: lsd_blur_resize_kernel, which
// tests/test_lsd_scale_plan_host.py compares as text — and this one is what the host checks the bound with.
STVO_BR_HD inline BrLayout br_tile_layout(int cmin, int cmax, int rmin, int rmax, int ntw, int nth, int hk, int tw, int th, int& nx_out,
                                          bool& xlist_out, bool& ylist_out, int& nr_out) {
    const int nx = cmax - cmin + 1, ny = rmax - rmin + 1;
    const bool xlist = nx > 2 * ntw, ylist = ny > 2 * nth;
    const int nr = ylist ? 2 * nth : ny;
    nx_out = nx; xlist_out = xlist; ylist_out = ylist; nr_out = nr;
    return br_layout(nx, ny, 4 * (((xlist ? 2 * ntw : nx) + 3) / 4), nr, hk, tw, th);
}

// The tile of the scaled image and the dynamic LDS of its launch: 64 x 16 unless the source window of such a tile (it grows with
// 1 / scale) exceeds the budget, then the longer side is halved; false: not even one output pixel per workgroup fits.
inline bool plan_blur_resize_u8(int scols, int srows, double scale, int radius, BlurResizePlan* p) {
    const double step = 1.0 / scale;
    for (int twl = 6, thl = 4;;) {
        const int tw = 1 << twl, th = 1 << thl;
        // first and last tap of a tile: floor() of positions (tile - 1) step apart, + 1 for the second tap, + 1 for the two floors,
        // + 1 for the roundings to float — never more than the image
        const double sx = std::ceil((tw - 1) * step) + 4, sy = std::ceil((th - 1) * step) + 4;
        const int nx = (int)(sx < scols ? sx : scols), ny = (int)(sy < srows ? sy : srows);
        // (a contiguous run is at most 2 tile columns rounded up to 4, the pairs are 2 per column)
        const int run = 4 * ((nx + 3) / 4), most = 2 * tw > 4 ? 2 * tw : 4;
        const int ncp = run < most ? run : most, nr = ny < 2 * th ? ny : 2 * th;
        const long long bytes = br_layout(nx, ny, ncp, nr, radius, tw, th).bytes;
        if (bytes <= BR_LDS_BUDGET) {
            p->tw_log = twl; p->th_log = thl; p->lds_bytes = (int)bytes;
            return true;
        }
        if (twl == 0 && thl == 0) return false;
        if (twl >= thl) --twl;
        else --thl;
    }
}

}  // namespace stvo
