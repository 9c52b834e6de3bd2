// frontend_layout.h — the device memory of the front-end objects (ORB, LBD, LSD, FLD, the rectifier, the colour entry points), each
// block stated ONCE as a function on the carver (carver.h): run on a null base it yields the bytes to allocate (Carver::off), run on
// the allocation the pointers.  The create functions and host-buffer entry points copy those pointers into the kernel argument
// structs; nothing else computes an offset.  Host-pure (g++ alone compiles it): tests/cpp/frontend_layout_host.cpp runs every layout
// here without a device, and tests/test_frontend_layout_host.py holds each against its buffer list.
#pragma once

#include "../../include/stvo_types.h"
#include "carver.h"

namespace stvo {

// ---- ORB ---------------------------------------------------------------------------------------------------------------------------
inline int orb_cand_cap(int cols, int rows) { return rows * cols / 4 + 64; }  // FAST candidates a level image can hold

struct OrbLevelBufs {
    uint8_t* blur;          // [B][rows][cols] of the level
    int32_t* hist;          // [B][256]
    uint32_t *cand, *hkey;  // [B][cand_cap] each (either score type may be chosen later: stvo_orb_set_score_type)
    int32_t* n_cand;        // [B]
    uint8_t* img;           // [B][rows][cols] the resized image (levels > 0), or nullptr
    // per-level outputs when there is more than one level (orb_concat_kernel assembles the result), or nullptr
    float *kp, *resp, *ang;  // [B][K][2], [B][K], [B][K]
    uint8_t* desc;           // [B][K][32]
    int32_t *n, *n_tot;      // [B]
};
struct OrbArena {
    int8_t* pattern;    // [1024] the pool of patch size 31
    int32_t* th_own;    // [B] stvo_orb_set_fast_thresholds
    int8_t* effective;  // [1024] + umax [64] of a descriptor setting other than (2, 31)
    OrbLevelBufs lev[STVO_ORB_MAX_LEVELS];
};
inline OrbArena carve_orb_arena(Carver& c, int B, int K, int nlevels, const int* cols, const int* rows) {
    const size_t nb = (size_t)B, nk = nb * K;
    OrbArena a{};
    a.pattern = c.take<int8_t>(1024);
    a.th_own = c.take<int32_t>(nb);
    a.effective = c.take<int8_t>(1024 + 64);
    for (int l = 0; l < nlevels; ++l) {
        const size_t px = nb * rows[l] * cols[l], ncand = nb * orb_cand_cap(cols[l], rows[l]);
        const bool multi = nlevels > 1;
        OrbLevelBufs& q = a.lev[l];
        q.blur = c.take<uint8_t>(px);
        q.hist = c.take<int32_t>(nb * 256);
        q.cand = c.take<uint32_t>(ncand);
        q.hkey = c.take<uint32_t>(ncand);
        q.n_cand = c.take<int32_t>(nb);
        q.img = l ? c.take<uint8_t>(px) : nullptr;
        q.kp = multi ? c.take<float>(nk * 2) : nullptr;
        q.resp = multi ? c.take<float>(nk) : nullptr;
        q.ang = multi ? c.take<float>(nk) : nullptr;
        q.desc = multi ? c.take<uint8_t>(nk * 32) : nullptr;
        q.n = multi ? c.take<int32_t>(nb) : nullptr;
        q.n_tot = multi ? c.take<int32_t>(nb) : nullptr;
    }
    return a;
}

// staging of stvo_orb_detect_levels: the images in, every result out (the results are zeroed per call: [kp, end of the block))
struct OrbStaging {
    uint8_t* img;
    float *kp, *resp, *ang;
    int32_t* oct;
    uint8_t* desc;
    int32_t *n, *n_total;
};
inline OrbStaging carve_orb_staging(Carver& c, int B, int cols, int rows, int K) {
    const size_t nb = (size_t)B, nk = nb * K;
    OrbStaging s;
    s.img = c.take<uint8_t>(nb * rows * cols);
    s.kp = c.take<float>(nk * 2); s.resp = c.take<float>(nk); s.ang = c.take<float>(nk); s.oct = c.take<int32_t>(nk);
    s.desc = c.take<uint8_t>(nk * 32); s.n = c.take<int32_t>(nb); s.n_total = c.take<int32_t>(nb);
    return s;
}

// ---- LBD ---------------------------------------------------------------------------------------------------------------------------
constexpr int LBD_DESC_FLOATS = 72;  // the float descriptor of a key-line (lbd_kernels.hip: LBD_DESC)

struct LbdArena {
    uint8_t* blur;  // [B][rows][cols]
    int32_t* dxy;   // [B][rows][cols] (dx, dy)
};
inline LbdArena carve_lbd_arena(Carver& c, int B, int cols, int rows) {
    const size_t px = (size_t)B * rows * cols;
    LbdArena a;
    a.blur = c.take<uint8_t>(px); a.dxy = c.take<int32_t>(px);
    return a;
}

// staging of stvo_lbd_compute: images, key-lines and counts in, both descriptors out (zeroed per call: [desc, end of the block)).  The
// float descriptor is cut whether or not a call asks for it.
struct LbdStaging {
    uint8_t* img;
    stvo_keyline* lines;
    int32_t* n;
    uint8_t* desc;
    float* desc_f;
};
inline LbdStaging carve_lbd_staging(Carver& c, int B, int cols, int rows, int M) {
    const size_t nb = (size_t)B, nl = nb * M;
    LbdStaging s;
    s.img = c.take<uint8_t>(nb * rows * cols); s.lines = c.take<stvo_keyline>(nl); s.n = c.take<int32_t>(nb);
    s.desc = c.take<uint8_t>(nl * 32); s.desc_f = c.take<float>(nl * LBD_DESC_FLOATS);
    return s;
}

// ---- LSD ---------------------------------------------------------------------------------------------------------------------------
// A pixel as the region growing sees it.  Three arrays (angle, (cos, sin), flag) were three divergent 64-lane gathers per sub-group
// and round, and the batches are bound by exactly that — the address path of a CU shared by its sixteen waves (SQ counters, round 6:
// the vector port of a SIMD is 29 % taken at four images per SIMD, a round takes 3.3 x as long as alone).
struct LsdPx {
    float ang;     // level-line angle in degrees, < 0: undefined
    float c, s;    // cos / sin of float(angle in radians) as floats: what the pixel adds to a region's direction sums
    int32_t used;  // 0 / 1: taken by a region (the only field written after lsd_gradient_kernel)
};
constexpr int LSD_UNIT_ROWS = 64;
constexpr int LSD_UNIT = 64 * LSD_UNIT_ROWS;  // pixels per wave of the pseudo-ordering's counting sort
constexpr int LSD_CTL = 512;                  // control words per image of lsd_grow_xcd_kernel, zeroed per call

// (the shapes are those of LsdDev, lsd_kernels.hip; img, lines, response and n_lines are the staging of the host-buffer entry points)
struct LsdArena {
    uint8_t* blur;  // [B][rows][cols] the blurred input of radius 3 (the fused kernel of the other radii keeps it in LDS), or nullptr
    uint8_t *scaled, *img;
    LsdPx* px;
    int32_t* k32;
    uint32_t *cnt, *order;
    int32_t *reg, *kmax;
    float4* seg;
    int32_t* n_seg;
    stvo_keyline* lines;
    float* response;
    int32_t *n_lines, *n_pass;
};
inline LsdArena carve_lsd_arena(Carver& c, int B, int cols, int rows, int w, int h, int n_bins, int seg_cap, int K, bool blur7) {
    const size_t nb = (size_t)B, in = nb * cols * rows, npx = (size_t)w * h;
    LsdArena a;
    a.blur = blur7 ? c.take<uint8_t>(in) : nullptr;
    a.scaled = c.take<uint8_t>(nb * npx); a.img = c.take<uint8_t>(in);
    a.px = c.take<LsdPx>(nb * npx); a.k32 = c.take<int32_t>(nb * npx);
    a.cnt = c.take<uint32_t>(nb * ((npx + LSD_UNIT - 1) / LSD_UNIT) * (size_t)n_bins);
    a.order = c.take<uint32_t>(nb * npx); a.reg = c.take<int32_t>(nb * npx); a.kmax = c.take<int32_t>(nb);
    a.seg = c.take<float4>(nb * seg_cap); a.n_seg = c.take<int32_t>(nb);
    a.lines = c.take<stvo_keyline>(nb * K); a.response = c.take<float>(nb * K); a.n_lines = c.take<int32_t>(nb); a.n_pass = c.take<int32_t>(nb);
    return a;
}

// lsd_grow_xcd_kernel serves small batches that do not refine: up to 16 images per XCD, each with a committer's workgroup + at least one
// speculating workgroup (~40 B of scratch per pixel and speculating workgroup); beyond that one wave per image and the batch as the
// parallelism.  The committer's bitmap (96 KB) + the feeder's ring + the per-wave scratch must fit the 160 KB of a CU.
constexpr int LSD_WAVES_MAX_B = 128;
constexpr size_t LSD_XCD_MAX_PX = 3u << 18;
inline bool lsd_xcd_route(int refine, int B, size_t npx) { return refine == 0 && B <= LSD_WAVES_MAX_B && npx <= LSD_XCD_MAX_PX; }

// scratch of lsd_grow_xcd_kernel, nw waves per image: cut only where lsd_xcd_route holds.  The control words lie right behind the
// pending table, inside its cut, so that one memset clears both; a call clears (stamp, stamp_bytes) and (pend, pend_ctl_bytes).
struct LsdXcdArena {
    int32_t *stamp, *wlist;  // [B][nw][w h] each
    long long* pend;         // [B][w h]
    int32_t* ctl;            // [B][LSD_CTL], unpadded behind pend
    size_t stamp_bytes, pend_ctl_bytes;
};
inline LsdXcdArena carve_lsd_xcd_arena(Carver& c, int B, size_t npx, size_t nw) {
    const size_t nb = (size_t)B;
    LsdXcdArena a;
    a.stamp_bytes = nb * nw * npx * 4;
    a.pend_ctl_bytes = nb * npx * 8 + nb * LSD_CTL * 4;
    a.stamp = c.take<int32_t>(nb * nw * npx); a.wlist = c.take<int32_t>(nb * nw * npx);
    char* pc = c.take<char>(a.pend_ctl_bytes);
    a.pend = reinterpret_cast<long long*>(pc);
    a.ctl = reinterpret_cast<int32_t*>(pc + nb * npx * 8);
    return a;
}

// ---- FLD ---------------------------------------------------------------------------------------------------------------------------
struct FldChain {
    int32_t seed, off, n, nseg;  // seed raster index, first point in pts, points, segments kept
};
constexpr int FLD_UNIT_ROWS = 64;
constexpr int FLD_UNIT = 64 * FLD_UNIT_ROWS;  // elements per wave of the counting sort
constexpr int FLD_BINS = 1024;                 // 10-bit digits of the root (images up to 2^20 pixels)
constexpr int FLD_SEG_CAP = 8192;              // segments per image in detection order (ranked); more are counted

// the words of the edge map, the units of the counting sort and the chain / segment stores of an image of npx pixels
inline int fld_words(int npx) { return (npx + 63) / 64 * 2; }
inline int fld_units(int npx) { return (npx + FLD_UNIT - 1) / FLD_UNIT; }
inline int fld_store_cap(int npx, int L) { return npx / (L + 1) + 1; }  // a kept chain holds at least L + 1 pixels; n points give at most n / (L + 1) segments

// (the shapes are those of FldDev, fld_kernels.hip; img, lines, response and n_lines are the staging of the host-buffer entry points)
struct FldArena {
    uint8_t* img;
    uint32_t *ebits, *sbits, *wsum;
    int32_t* lab;
    uint32_t *tmp, *list, *cnt;
    int32_t* n_edge;
    uint32_t* pts;
    int32_t* ch_at;
    FldChain* ch;
    int32_t* n_ch;
    float4 *sg, *dseg;
    int32_t *n_seg, *err;
    stvo_keyline* lines;
    float* response;
    int32_t* n_lines;
};
inline FldArena carve_fld_arena(Carver& c, int B, int cols, int rows, int L, int K) {
    const int ipx = cols * rows;
    const size_t nb = (size_t)B, npx = (size_t)ipx, nw = (size_t)fld_words(ipx), cap = (size_t)fld_store_cap(ipx, L);
    FldArena a;
    a.img = c.take<uint8_t>(nb * npx);
    a.ebits = c.take<uint32_t>(nb * nw); a.sbits = c.take<uint32_t>(nb * nw); a.wsum = c.take<uint32_t>(nb * nw);
    a.lab = c.take<int32_t>(nb * npx); a.tmp = c.take<uint32_t>(nb * npx); a.list = c.take<uint32_t>(nb * npx);
    a.cnt = c.take<uint32_t>(nb * fld_units(ipx) * FLD_BINS); a.n_edge = c.take<int32_t>(nb);
    a.pts = c.take<uint32_t>(nb * npx); a.ch_at = c.take<int32_t>(nb * npx);
    a.ch = c.take<FldChain>(nb * cap); a.n_ch = c.take<int32_t>(nb);
    a.sg = c.take<float4>(nb * cap); a.dseg = c.take<float4>(nb * FLD_SEG_CAP); a.n_seg = c.take<int32_t>(nb); a.err = c.take<int32_t>(nb);
    a.lines = c.take<stvo_keyline>(nb * K); a.response = c.take<float>(nb * K); a.n_lines = c.take<int32_t>(nb);
    return a;
}

// ---- the rectifier and the colour entry points: staging of the host-buffer calls -------------------------------------------------------
// Two sources in, two destinations out.
struct StereoStaging {
    uint8_t *src_l, *src_r, *dst_l, *dst_r;
};
// stvo_rectify_images: four sides of B images back to back, UNPADDED inside one cut — a side begins where the remap kernel has always
// seen it, whatever B cols rows is a multiple of
inline StereoStaging carve_rectify_staging(Carver& c, int B, int cols, int rows) {
    const size_t side = (size_t)B * cols * rows;
    uint8_t* p = c.take<uint8_t>(4 * side);
    return StereoStaging{p, p + side, p + 2 * side, p + 3 * side};
}
// stvo_rectify_color_images: four sides of the n images of the call, each a cut of its own
inline StereoStaging carve_color_rectify_staging(Carver& c, int n, int cols, int rows, int channels) {
    const size_t bytes = (size_t)n * cols * rows * channels;
    StereoStaging s;
    s.src_l = c.take<uint8_t>(bytes); s.src_r = c.take<uint8_t>(bytes); s.dst_l = c.take<uint8_t>(bytes); s.dst_r = c.take<uint8_t>(bytes);
    return s;
}
// stvo_color_to_gray: the colour batch, then two planes (the second is cut whether or not a call asks for it)
struct GrayStaging {
    uint8_t *src, *gray, *swapped;
};
inline GrayStaging carve_gray_staging(Carver& c, size_t npix, int channels) {
    GrayStaging s;
    s.src = c.take<uint8_t>(npix * channels); s.gray = c.take<uint8_t>(npix); s.swapped = c.take<uint8_t>(npix);
    return s;
}

}  // namespace stvo
