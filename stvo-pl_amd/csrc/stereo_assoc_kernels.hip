// stereo_assoc_kernels.hip — the stereo association of one frame of B sequences into the stereo set being built (SeqDev::cur): stages
// 1, 3, 4 and 6 of the device-resident pipeline (seq_pipeline.hip lists them) and the fused key-line stage 4 + 5 + 6.  Line numbers
// without a file are src/stereoFrame.cpp of the reference.  The launchers at the end are declared in kernels.h.
#include "point_cells.h"
#include "pose_math.h"
#include "seq_state.h"

// The geometry filters of the tail kernels decide on thresholds (min_disp, ls_min_disp_ratio, stereo_overlap_th): no
// fused multiply-adds, so that they round exactly like the reference's separate operations (and like the host mirror,
// which is built with -ffp-contract=off).
#pragma clang fp contract(off)

namespace stvo {
namespace {

__device__ __forceinline__ bool in_grid(int x, int y) {
    return x >= 0 && x < STVO_GRID_COLS && y >= 0 && y < STVO_GRID_ROWS;
}

// exclusive scan of hist[0..256 * PER) in LDS by 256 threads (PER cells each); writes start[0..256 * PER]
template <int PER, typename T>
__device__ __forceinline__ void scan_cells_n(T* hist, int* s_wave, int32_t* start_out) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int local[PER];
    int sum = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        local[k] = hist[tid * PER + k];
        sum += local[k];
    }
    int incl = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(incl, o, 64);
        if (lane >= o) incl += v;
    }
    if (lane == 63) s_wave[wv] = incl;
    __syncthreads();
    int base = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w)
        if (w < wv) base += s_wave[w];
    int run = base + incl - sum;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        hist[tid * PER + k] = (T)run;  // hist becomes the exclusive start
        start_out[tid * PER + k] = run;
        run += local[k];
    }
    if (tid == 255) start_out[256 * PER] = run;
    __syncthreads();
}
template <typename T>
__device__ __forceinline__ void scan_cells(T* hist, int* s_wave, int32_t* start_out) {
    scan_cells_n<STVO_GRID_CELLS / 256>(hist, s_wave, start_out);
}

// ---- 1: points — cells + CSR of the right key-points (point_cells.h) -------------------------------
// (16-bit counters — half the LDS, so that line workgroups fit beside this kernel's — gained 0.7 % on 1024 KITTI-shaped streams and
// lost 10 % on 512 EuRoC-shaped ones, where the line stream is the longer one and every speed-up of the point stream takes CUs from it)
template <bool LEAN>
__global__ __launch_bounds__(256) void point_cells_kernel(SeqDev s) {
    __shared__ PointCellsLds<256> lds;
    point_cells_frame<256, LEAN>(point_cells_args(s), blockIdx.x, &lds);
}

// ---- 3: points — filters, back-projection, ordered compaction ---------------------------------------
// 1024 threads per frame: the compaction offset is carried from chunk to chunk (three barriers each), so fewer, larger
// chunks shorten the chain — 2 chunks instead of 8 for ~2000 key-points.
constexpr int TAIL_BLOCK = 1024;
__global__ __launch_bounds__(TAIL_BLOCK) void point_tail_kernel(SeqDev s) {
    __shared__ int s_wave[TAIL_BLOCK / 64];
    __shared__ int s_run;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int nl = s.raw.n_kp_l[b];
    const size_t off = (size_t)b * s.K;
    const PointTail t = point_tail_args(s);
    if (tid == 0) s_run = 0;
    __syncthreads();
    for (int base = 0; base < nl; base += TAIL_BLOCK) {
        const int i = base + tid;
        bool ok = false;
        double disp = 0.0;
        if (i < nl) {
            const int i2 = s.m12s_p[off + i];
            if (i2 >= 0) ok = point_tail_filter(t, off, i, i2, disp);
        }
        // ordered compaction: stereo_pt / pdesc_l keep ascending left index (:161-172)
        const unsigned long long bal = __ballot(ok);
        const int before = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) s_wave[wv] = __popcll(bal);
        __syncthreads();
        int wbase = s_run;
        for (int w = 0; w < wv; ++w) wbase += s_wave[w];
        if (ok) point_tail_write(t, off, i, off + (size_t)(wbase + before), disp);
        __syncthreads();
        if (tid == 0) {
            int q = 0;
            for (int w = 0; w < TAIL_BLOCK / 64; ++w) q += s_wave[w];
            s_run += q;
        }
        __syncthreads();
    }
    if (tid == 0) {
        s.cur.n[b] = s_run;
        if (s.host_n) s.host_n[b] = s_run;
        if (s.zero_nl) s.cur.nl[b] = 0;
    }
}

// LineIterator (src/lineIterator.cpp:34-77): calls f(x, y) for every Bresenham cell
template <typename F>
__device__ __forceinline__ void bresenham(double x1, double y1, double x2, double y2, F f) {
    const bool steep = fabs(y2 - y1) > fabs(x2 - x1);
    double t;
    if (steep) {
        t = x1; x1 = y1; y1 = t;
        t = x2; x2 = y2; y2 = t;
    }
    if (x1 > x2) {
        t = x1; x1 = x2; x2 = t;
        t = y1; y1 = y2; y2 = t;
    }
    const double dx = x2 - x1, dy = fabs(y2 - y1);
    double error = dx / 2.0;
    const int ystep = (y1 < y2) ? 1 : -1;
    int y = (int)y1;
    const int maxX = (int)x2;
    int guard = 0;
    for (int x = (int)x1; x <= maxX && guard < LENT; ++x, ++guard) {
        f(steep ? y : x, steep ? x : y);
        error -= dy;
        if (error < 0) {
            y += ystep;
            error += dx;
        }
    }
}

// ---- 4: lines — end-point cells, rasterised CSR of the right lines, directions ----------------------
__global__ __launch_bounds__(256) void line_cells_kernel(SeqDev s) {
    __shared__ int hist[STVO_GRID_CELLS];
    __shared__ int fill[STVO_GRID_CELLS];
    __shared__ int s_wave[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int nl = s.raw.n_kl_l[b], nr = s.raw.n_kl_r[b];
    const size_t off = (size_t)b * s.M;
    const double inv_w = s.inv_wh[2 * b], inv_h = s.inv_wh[2 * b + 1];
    for (int i = tid; i < nl; i += 256) {  // :318-322
        const float* kl = s.raw.kl_l + (off + i) * 4;
        s.lxy_l[(off + i) * 4 + 0] = (int)((double)kl[0] * inv_w);
        s.lxy_l[(off + i) * 4 + 1] = (int)((double)kl[1] * inv_h);
        s.lxy_l[(off + i) * 4 + 2] = (int)((double)kl[2] * inv_w);
        s.lxy_l[(off + i) * 4 + 3] = (int)((double)kl[3] * inv_h);
    }
    for (int c = tid; c < STVO_GRID_CELLS; c += 256) {
        hist[c] = 0;
        fill[c] = 0;
    }
    __syncthreads();
    for (int j = tid; j < nr; j += 256) {  // :325-338
        const float* kl = s.raw.kl_r + (off + j) * 4;
        const double vx = (double)(kl[2] - kl[0]) * inv_w;  // float difference, then * double (:331)
        const double vy = (double)(kl[3] - kl[1]) * inv_h;
        const double mag = sqrt(vx * vx + vy * vy);
        s.ldir[(off + j) * 2 + 0] = vx / mag;
        s.ldir[(off + j) * 2 + 1] = vy / mag;
        s.lperm[off + j] = j;  // few lines: identity scan order
        s.lrank[off + j] = j;
        bresenham((double)kl[0] * inv_w, (double)kl[1] * inv_h, (double)kl[2] * inv_w, (double)kl[3] * inv_h,
                  [&](int x, int y) {
                      if (in_grid(x, y)) atomicAdd(&hist[y * STVO_GRID_COLS + x], 1);
                  });
    }
    __syncthreads();
    scan_cells(hist, s_wave, s.lstart + (size_t)b * (STVO_GRID_CELLS + 1));
    int32_t* items = s.litems + (size_t)b * s.M * LENT;
    for (int j = tid; j < nr; j += 256) {
        const float* kl = s.raw.kl_r + (off + j) * 4;
        bresenham((double)kl[0] * inv_w, (double)kl[1] * inv_h, (double)kl[2] * inv_w, (double)kl[3] * inv_h,
                  [&](int x, int y) {
                      if (in_grid(x, y)) {
                          const int c = y * STVO_GRID_COLS + x;
                          items[hist[c] + atomicAdd(&fill[c], 1)] = j;
                      }
                  });
    }
}

// ---- 6: lines — geometry filters, back-projection, ordered compaction --------------------------------
// the tail of frame b by a workgroup of T threads; match_of(i) = stereo match of left line i (the caller has put a barrier
// after s_run = 0 and after whatever match_of reads)
template <int T, typename MatchOf>
__device__ __forceinline__ void line_tail_frame(const SeqDev& s, const int b, MatchOf match_of, int* s_wave, int* s_run) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int nl = s.raw.n_kl_l[b];
    const size_t off = (size_t)b * s.M;
    const stvo_cam cam = s.cams[b];
    for (int base = 0; base < nl; base += T) {
        const int i = base + tid;
        bool ok = false;
        double sp_l[2] = {0, 0}, ep_l[2] = {0, 0}, le_l[3] = {0, 0, 0}, disp_s = 0.0, disp_e = 0.0;
        if (i < nl) {
            const int i2 = match_of(i);
            if (i2 >= 0) {
                const float* l = s.raw.kl_l + (off + i) * 4;
                const float* r = s.raw.kl_r + (off + i2) * 4;
                sp_l[0] = (double)l[0]; sp_l[1] = (double)l[1];
                ep_l[0] = (double)l[2]; ep_l[1] = (double)l[3];
                // le_l = sp_l x ep_l (homogeneous, w = 1), normalised by |(l0, l1)|   (:353-355)
                le_l[0] = sp_l[1] - ep_l[1];
                le_l[1] = ep_l[0] - sp_l[0];
                le_l[2] = sp_l[0] * ep_l[1] - sp_l[1] * ep_l[0];
                const double nrm = sqrt(le_l[0] * le_l[0] + le_l[1] * le_l[1]);
                le_l[0] /= nrm; le_l[1] /= nrm; le_l[2] /= nrm;
                double sp_r[2] = {(double)r[0], (double)r[1]}, ep_r[2] = {(double)r[2], (double)r[3]};
                const double overlap = pm::stereo_row_overlap(sp_l[1], ep_l[1], sp_r[1], ep_r[1], s.mp.line_horiz_th);
                // :363-364 — the second line reads the ALREADY overwritten sp_r (reference quirk, kept)
                sp_r[0] = (sp_r[0] * (sp_l[1] - ep_r[1]) + ep_r[0] * (sp_r[1] - sp_l[1])) / (sp_r[1] - ep_r[1]);
                sp_r[1] = sp_l[1];
                ep_r[0] = (sp_r[0] * (ep_l[1] - ep_r[1]) + ep_r[0] * (sp_r[1] - ep_l[1])) / (sp_r[1] - ep_r[1]);
                ep_r[1] = ep_l[1];
                pm::stereo_line_disparities(sp_l[0], ep_l[0], sp_r[0], ep_r[0], s.mp.ls_min_disp_ratio, &disp_s, &disp_e);  // :405-415
                ok = disp_s >= s.mp.min_disp && disp_e >= s.mp.min_disp && fabs(sp_l[1] - ep_l[1]) > s.mp.line_horiz_th &&
                     fabs(sp_r[1] - ep_r[1]) > s.mp.line_horiz_th && overlap > s.mp.stereo_overlap_th;
            }
        }
        const unsigned long long bal = __ballot(ok);
        const int before = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) s_wave[wv] = __popcll(bal);
        __syncthreads();
        int wbase = (*s_run);
        for (int w = 0; w < wv; ++w) wbase += s_wave[w];
        if (ok) {
            const size_t k = off + (size_t)(wbase + before);
            const double bds = cam.b / disp_s, bde = cam.b / disp_e;
            s.cur.spl[k * 2 + 0] = sp_l[0]; s.cur.spl[k * 2 + 1] = sp_l[1];
            s.cur.epl[k * 2 + 0] = ep_l[0]; s.cur.epl[k * 2 + 1] = ep_l[1];
            s.cur.sP[k * 3 + 0] = bds * (sp_l[0] - cam.cx);
            s.cur.sP[k * 3 + 1] = bds * (sp_l[1] - cam.cy);
            s.cur.sP[k * 3 + 2] = bds * cam.fx;
            s.cur.eP[k * 3 + 0] = bde * (ep_l[0] - cam.cx);
            s.cur.eP[k * 3 + 1] = bde * (ep_l[1] - cam.cy);
            s.cur.eP[k * 3 + 2] = bde * cam.fx;
            s.cur.le[k * 3 + 0] = le_l[0]; s.cur.le[k * 3 + 1] = le_l[1]; s.cur.le[k * 3 + 2] = le_l[2];
            const int level = s.raw.oct_ll[off + i];
            double sg = 1.0;  // LineFeature ctor (src/stereoFeatures.cpp:107-115)
            for (int t = 0; t < level; ++t) sg *= s.mp.lsd_scale;
            const double s2 = 1.0 / (sg * sg);
            s.cur.s2l[k] = s2;
            double sm = s2;  // LineFeature::safeCopy re-applies the level scaling (:117-135)
            for (int t = 0; t < level; ++t) sm *= s.mp.lsd_scale;
            s.cur.s2lm[k] = 1.0 / (sm * sm);
            const uint4* src = reinterpret_cast<const uint4*>(s.raw.ldesc_l + (off + i) * STVO_DESC_BYTES);
            uint4* dst = reinterpret_cast<uint4*>(s.cur.ldesc + k * STVO_DESC_BYTES);
            dst[0] = src[0];
            dst[1] = src[1];
        }
        __syncthreads();
        if (tid == 0)
            for (int w = 0; w < T / 64; ++w) (*s_run) += s_wave[w];
        __syncthreads();
    }
    if (tid == 0) {
        s.cur.nl[b] = *s_run;
        if (s.host_nl) s.host_nl[b] = *s_run;
    }
}

__global__ __launch_bounds__(256) void line_tail_kernel(SeqDev s) {
    __shared__ int s_wave[4];
    __shared__ int s_run;
    const int b = blockIdx.x;
    const size_t off = (size_t)b * s.M;
    if (threadIdx.x == 0) s_run = 0;
    __syncthreads();
    line_tail_frame<256>(s, b, [&](int i) { return s.m12s_l[off + i]; }, s_wave, &s_run);
}

// ---- 4 + 5 + 6 in one workgroup per frame: the whole stereo association of the key-lines --------------------------------------
// A frame holds ~100 key-lines (lsd_nfeatures 100 / 300).  Through the general grid machinery (CSR of the rasterised right lines,
// candidate bit-matrix, scan / elig / scan / finalize, tail: seven launches, a thread or a wave per line) the stage took ~290 us
// per 1024 frames on an idle GPU and, sharing the CUs with the key-point stage, stretched that stage and the key-point scan by
// ~0.1 ms.  Here thread j owns RIGHT line j: it rasterises the line once into per-grid-row column intervals in LDS (a Bresenham
// line covers one contiguous run of columns in every row it crosses), and the candidates of left line i1 — the right lines with a
// cell in the window of either END-POINT cell of i1 (src/matching.cpp:213-215; window = matching_s_ws columns to the left, same
// row, stereoFrame.cpp:340-342) — become two interval tests.  matchGrid's order dependence (:145-150: a pair takes part only if it
// strictly improves on every earlier left line that met the same right line) is local to thread j, which walks i1 in ascending
// order; the best of a left line is an LDS atomic min over (distance << 16 | j), the ratio test (:241, DOUBLE) a second walk, the
// mutual check (:247-255) one thread per left line.  Left lines, directions and descriptors are read through wave-uniform LDS
// addresses (broadcasts).  Ties: the best of two equal distances fails the ratio test for ratios <= 1 whichever is "first".
// The columns [cmin, cmax] of a right line in a grid row are kept as the bytes cmin | (255 - cmax) << 8 and read into two 16-bit
// lanes (one v_perm_b32); the window [lo, hi] of a left end-point is hi | (255 - lo) << 16: the intervals meet iff both lanes of
// (window - run) are >= 0 — a permute, one packed subtraction and a mask per (end-point, right line) instead of two byte extractions
// and four comparisons (the candidate matrix is about two thirds of this kernel's instructions).  (The same with 32-bit entries, no
// permute: SLOWER — 0.845 -> 0.853 ms per 1024 KITTI-shaped streams, 0.470 -> 0.598 ms per 512 EuRoC-shaped ones: the LDS the kernel
// asks for, i.e. how many of its workgroups a CU holds, weighs more than its instruction count.)
constexpr uint32_t LSF_ROW_EMPTY = 0xFFFFu;      // cmin = 255 > cmax = 0
constexpr uint32_t LSF_NO_WINDOW = 0x0000FFFFu;  // hi = -1: below every cmin
// (LSF_MAX_LINES and LSF_BYTES_PER_LINE, what a launch is sized with: step_plan.h)
// Mk (<= s.M): lines per image the LDS arrays are sized for — the host knows that no image of the batch holds more.
// T: threads per frame (256; a single wave per frame was tried to hold fewer wave slots, and was slower).
template <int T>
__global__ __launch_bounds__(T) void line_stereo_fused_kernel(SeqDev s, const int Mk, const int mutual, const double ratio) {
    extern __shared__ uint4 s_dyn[];
    __shared__ int s_wave[4];
    __shared__ int s_run;
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const int M = Mk, b = blockIdx.x, tid = threadIdx.x;
    u32x4* dl = reinterpret_cast<u32x4*>(s_dyn);                                      // [M][2] left descriptor rows
    int4* cxy = reinterpret_cast<int4*>(dl + 2 * M);                                  // [M] windows of the two end-point cells of the left lines: (grid row * M, packed window) twice
    double2* vdir = reinterpret_cast<double2*>(cxy + M);                              // [M] their unit directions (integer cell differences)
    uint32_t* best = reinterpret_cast<uint32_t*>(vdir + M);                           // [M] min (d << 16 | j) over the eligible pairs
    unsigned short* rows = reinterpret_cast<unsigned short*>(best + M);               // [48][M] cmin | (255 - cmax) << 8 of right line j in grid row y
    unsigned short* owner = rows + (size_t)STVO_GRID_ROWS * M;                        // [M] matches_21
    short* mm = reinterpret_cast<short*>(owner + M);                                  // [M] the stereo match of left line i
    unsigned char* blocked = reinterpret_cast<unsigned char*>(mm + M);                // [M] ratio test failed
    uint32_t* cand = reinterpret_cast<uint32_t*>(blocked + M + ((4 - (M & 3)) & 3));  // [M / 32][M] bit k of word (w, j): left line 32 w + k has right line j as a candidate
    const int nl = min(s.raw.n_kl_l[b], M), nr = min(s.raw.n_kl_r[b], M);
    const size_t off = (size_t)b * s.M;
    const double inv_w = s.inv_wh[2 * b], inv_h = s.inv_wh[2 * b + 1];
    const int ws = s.mp.matching_s_ws;
    const double sim_th = s.mp.line_sim_th;
    if (tid == 0) s_run = 0;
    for (int i = tid; i < nl; i += T) {  // :318-322, include/matching.h:48-53
        const float* kl = s.raw.kl_l + (off + i) * 4;
        int4 c;
        c.x = (int)((double)kl[0] * inv_w);
        c.y = (int)((double)kl[1] * inv_h);
        c.z = (int)((double)kl[2] * inv_w);
        c.w = (int)((double)kl[3] * inv_h);
        // GridStructure::get(x, y, {ws, 0, 0, 0}): columns max(x - ws, 0) .. min(x, 63) of row y (nothing outside the grid's rows)
        auto window = [&](int x, int y, int& row_off, int& q) {
            const bool row_ok = y >= 0 && y < STVO_GRID_ROWS;
            const int lo = max(x - ws, 0), hi = min(x, STVO_GRID_COLS - 1);
            row_off = (row_ok ? y : 0) * M;
            q = (row_ok && lo <= hi) ? (int)((uint32_t)hi | ((uint32_t)(255 - lo) << 16)) : (int)LSF_NO_WINDOW;
        };
        int4 wq;
        window(c.x, c.y, wq.x, wq.y);
        window(c.z, c.w, wq.z, wq.w);
        cxy[i] = wq;
        const double vx = (double)(c.z - c.x), vy = (double)(c.w - c.y);
        const double mag = sqrt(vx * vx + vy * vy);
        vdir[i] = make_double2(vx / mag, vy / mag);  // 0 / 0 = NaN never skips a candidate (:207-222)
        const u32x4* g = reinterpret_cast<const u32x4*>(s.raw.ldesc_l + (off + i) * STVO_DESC_BYTES);
        dl[2 * i] = g[0];
        dl[2 * i + 1] = g[1];
        best[i] = 0xFFFFFFFFu;
        blocked[i] = 0;
    }
    for (int j = tid; j < nr; j += T) {  // :325-338
        for (int y = 0; y < STVO_GRID_ROWS; ++y) rows[y * M + j] = (unsigned short)LSF_ROW_EMPTY;
        const float* kl = s.raw.kl_r + (off + j) * 4;
        // the cells come row by row (the minor coordinate of a Bresenham walk is monotone): the run of the current row stays in
        // registers and is written once — no read-modify-write chain through LDS
        int cy = -1, cmn = 255, cmx = 0;
        auto flush = [&]() {
            if (cy >= 0 && cy < STVO_GRID_ROWS && cmn <= cmx) rows[cy * M + j] = (unsigned short)(cmn | ((255 - cmx) << 8));
        };
        bresenham((double)kl[0] * inv_w, (double)kl[1] * inv_h, (double)kl[2] * inv_w, (double)kl[3] * inv_h, [&](int x, int y) {
            if (y != cy) {
                flush();
                cy = y;
                cmn = 255;
                cmx = 0;
            }
            if (x >= 0 && x < STVO_GRID_COLS) {
                cmn = min(cmn, x);
                cmx = max(cmx, x);
            }
        });
        flush();
    }
    __syncthreads();
    // has right line j a cell in the window?  Both 16-bit lanes of (window - run) non-negative: cmin <= hi and lo <= cmax
    typedef short i16x2 __attribute__((ext_vector_type(2)));
    auto in_window = [&](int j, int row_off, int q) -> bool {
        const uint32_t run = __builtin_amdgcn_perm(0u, (uint32_t)rows[row_off + j], 0x0c010c00u);  // bytes (cmin, 255 - cmax) -> 16-bit lanes
        const i16x2 d = __builtin_bit_cast(i16x2, q) - __builtin_bit_cast(i16x2, run);
        return (__builtin_bit_cast(uint32_t, d) & 0x80008000u) == 0u;
    };
    // candidate bit-matrix, all threads: word (w, j) = left lines 32 w .. 32 w + 31 that have right line j as a candidate.  The
    // pairs are independent (the loads of one trip do not wait for the trip before), and the walks below then visit the few
    // candidates of a right line instead of testing every left line in a chain of dependent LDS reads.
    const int words = (nl + 31) >> 5;
    for (int e = tid; e < words * M; e += T) {
        const int w = e / M, j = e - w * M;
        uint32_t bits = 0u;
        if (j < nr) {
            const int i_end = min(32, nl - 32 * w);
#pragma unroll 4
            for (int k = 0; k < i_end; ++k) {
                const int4 c = cxy[32 * w + k];
                if (in_window(j, c.x, c.y) || in_window(j, c.z, c.w)) bits |= 1u << k;  // (row offset, window) of either end point
            }
        }
        cand[e] = bits;
    }
    __syncthreads();
    // the walk of thread j over its candidates in ascending left index; f(i1, d) is called for every eligible pair
    auto walk = [&](int j, const u32x4 t0, const u32x4 t1, const double dirx, const double diry, auto f) {
        int run_min = 0x7FFFFFFF;
        for (int w = 0; w < words; ++w) {
            for (uint32_t bits = cand[w * M + j]; bits; bits &= bits - 1u) {
                const int i1 = 32 * w + __builtin_ctz(bits);
                const double2 v = vdir[i1];
                const double dot = v.x * dirx + v.y * diry;
                if (fabs(dot) < sim_th) continue;  // :221-222
                const u32x4 q0 = dl[2 * i1], q1 = dl[2 * i1 + 1];
                const int d = __builtin_popcount(q0.x ^ t0.x) + __builtin_popcount(q0.y ^ t0.y) + __builtin_popcount(q0.z ^ t0.z) +
                              __builtin_popcount(q0.w ^ t0.w) + __builtin_popcount(q1.x ^ t1.x) + __builtin_popcount(q1.y ^ t1.y) +
                              __builtin_popcount(q1.z ^ t1.z) + __builtin_popcount(q1.w ^ t1.w);
                if (mutual) {  // :145-150 running strict minimum per right line
                    if (d >= run_min) continue;
                    run_min = d;
                }
                f(i1, d);
            }
        }
    };
    auto right_line = [&](int j, u32x4& t0, u32x4& t1, double& dirx, double& diry) {
        const float* kl = s.raw.kl_r + (off + j) * 4;
        const double vx = (double)(kl[2] - kl[0]) * inv_w;  // float difference, then * double (:331)
        const double vy = (double)(kl[3] - kl[1]) * inv_h;
        const double mag = sqrt(vx * vx + vy * vy);
        dirx = vx / mag;
        diry = vy / mag;
        const u32x4* g = reinterpret_cast<const u32x4*>(s.raw.ldesc_r + (off + j) * STVO_DESC_BYTES);
        t0 = g[0];
        t1 = g[1];
    };
    for (int j = tid; j < nr; j += T) {
        u32x4 t0, t1;
        double dirx, diry;
        right_line(j, t0, t1, dirx, diry);
        int own = 0xFFFF;
        walk(j, t0, t1, dirx, diry, [&](int i1, int d) {
            own = i1;
            atomicMin(&best[i1], ((uint32_t)d << 16) | (uint32_t)j);
        });
        owner[j] = (unsigned short)own;
    }
    __syncthreads();
    for (int j = tid; j < nr; j += T) {  // :241 for every eligible pair that is not its left line's best
        u32x4 t0, t1;
        double dirx, diry;
        right_line(j, t0, t1, dirx, diry);
        walk(j, t0, t1, dirx, diry, [&](int i1, int d) {
            const uint32_t bk = best[i1];
            if (bk != (((uint32_t)d << 16) | (uint32_t)j)) {
                const double best_d = (double)(int)(bk >> 16), d2 = (double)d;
                if (!(best_d < d2 * ratio)) blocked[i1] = 1;
            }
        });
    }
    __syncthreads();
    for (int i1 = tid; i1 < s.M; i1 += T) {  // accept, mutual check (:247-255)
        int m = -1;
        if (i1 < nl) {
            const uint32_t bk = best[i1];
            if (bk != 0xFFFFFFFFu && !blocked[i1] && (double)(int)(bk >> 16) < 2147483647.0 * ratio) {
                const int j = (int)(bk & 0xFFFFu);
                if (!mutual || (int)owner[j] == i1) m = j;
            }
        }
        if (i1 < M) mm[i1] = (short)m;
        const_cast<int32_t*>(s.m12s_l)[off + i1] = m;
    }
    __syncthreads();
    // (left lines beyond the LDS arrays — only possible if the launch was sized for fewer lines than the slot holds — are unmatched,
    //  never read out of bounds)
    line_tail_frame<T>(s, b, [&](int i) { return i < M ? (int)mm[i] : -1; }, s_wave, &s_run);
}
}  // namespace

void launch_point_cells(hipStream_t q, const SeqDev& d, bool lean) {
    if (lean)
        hipLaunchKernelGGL(point_cells_kernel<true>, dim3(d.B), dim3(256), 0, q, d);
    else
        hipLaunchKernelGGL(point_cells_kernel<false>, dim3(d.B), dim3(256), 0, q, d);
}
void launch_point_tail(hipStream_t q, const SeqDev& d) { hipLaunchKernelGGL(point_tail_kernel, dim3(d.B), dim3(TAIL_BLOCK), 0, q, d); }
void launch_line_cells(hipStream_t q, const SeqDev& d) { hipLaunchKernelGGL(line_cells_kernel, dim3(d.B), dim3(256), 0, q, d); }
void launch_line_tail(hipStream_t q, const SeqDev& d) { hipLaunchKernelGGL(line_tail_kernel, dim3(d.B), dim3(256), 0, q, d); }
// (one wave per frame, <64>: 185 instead of 150 us beside the key-point scan, which it stretched by 15 us more)
void launch_line_stereo_fused(hipStream_t q, const SeqDev& d, int lds_bytes, int Mk, int mutual, double ratio) {
    hipLaunchKernelGGL(line_stereo_fused_kernel<256>, dim3(d.B), dim3(256), lds_bytes, q, d, Mk, mutual, ratio);
}
bool line_stereo_fused_lds_opt_in(int lds_bytes) { return lds_opt_in(reinterpret_cast<const void*>(line_stereo_fused_kernel<256>), lds_bytes); }

}  // namespace stvo
