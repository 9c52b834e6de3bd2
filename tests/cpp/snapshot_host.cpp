// The product's stream snapshot (stvo-pl_amd/csrc/stream_snapshot.h: layout, header check, plain C++ pack / unpack) and the planner's
// import fact (step_plan.h) compiled for the host, behind a flat C interface — TEST INFRASTRUCTURE ONLY.
// tests/test_stream_snapshot_host.py names the entries of the arrays in the same order.
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../stvo-pl_amd/csrc/step_plan.h"
#include "../../stvo-pl_amd/csrc/stream_snapshot.h"

using namespace stvo;

extern "C" {

// out[NSEC + 1]: the offset of every section (-1: not cut), then bytes.  Returns NSEC + 1, or -1 for an illegal request.
int snh_layout(int K, int M, int flags, long long* out) {
    stvo_snapshot_layout l;
    if (!snap::layout(K, M, flags, l)) return -1;
    for (int i = 0; i < snap::NSEC; ++i) out[i] = snap::offsets(l)[i];
    out[snap::NSEC] = l.bytes;
    return snap::NSEC + 1;
}

// out[NSEC][4]: row_bytes, rows (0 one, 1 K, 2 M), count, flag of every section
int snh_sections(int* out) {
    for (int i = 0; i < snap::NSEC; ++i) {
        const snap::SectionDef& d = snap::SECTIONS[i];
        out[4 * i] = d.row_bytes; out[4 * i + 1] = d.rows; out[4 * i + 2] = d.count; out[4 * i + 3] = d.flag;
    }
    return snap::NSEC;
}

// bytes of a stereo set per stream as seq_layout.h cuts it at B = 1 (without the counts), for the comparison with the section sizes
long long snh_stereo_set_bytes(int K, int M) {
    Carver c(nullptr);
    (void)carve_stereo_set(c, 1, K, M, false);
    return (long long)c.off;
}

static stvo_cam cam0() { return stvo_cam{718.856, 718.856, 607.1928, 185.2157, 0.5372}; }
static snap::Target target0(int K, int M, int flags) {
    snap::Target t;
    std::memset(&t, 0, sizeof(t));
    t.K = K; t.M = M; t.flags = flags; t.cam = cam0(); t.cols = 1241; t.rows = 376;
    t.mp.matching_s_ws = 10; t.mp.min_ratio_12_p = 0.75f; t.mp.max_dist_epip = 1.0;
    t.op.has_points = 1; t.op.has_lines = 1; t.op.max_iters = 5; t.op.inlier_k = 4.0;
    return t;
}
static snap::Header header0(int K, int M, int flags, int n, int nl, int kf_n, int kf_nl) {
    const snap::Target t = target0(K, M, flags);
    stvo_snapshot_layout l;
    snap::layout(K, M, flags, l);
    snap::Header h;
    std::memset(&h, 0, sizeof(h));
    h.magic = snap::MAGIC; h.version = snap::VERSION; h.bytes = l.bytes; h.K = K; h.M = M; h.flags = flags; h.n = n; h.nl = nl;
    if (flags & STVO_SNAP_KF_SETS) h.kf = stvo_kf_header{kf_n, kf_nl, 7, 2};
    h.cam = t.cam; h.cols = t.cols; h.rows = t.rows; h.mp = t.mp; h.op = t.op;
    return h;
}

// check_header of a well-formed header of an exporter (K, M, flags, counts) with ONE field broken (what), against a target pipeline
// (Kt, Mt, flags).  what: 0 nothing, 1 magic, 2 version, 3 bytes, 4 flags of the target differ, 5 camera, 6 image size, 7 mp, 8 op,
// 9 blob_stride one short of bytes.
int snh_check(int K, int M, int flags, int n, int nl, int kf_n, int kf_nl, int Kt, int Mt, int what) {
    snap::Header h = header0(K, M, flags, n, nl, kf_n, kf_nl);
    snap::Target t = target0(Kt, Mt, flags);
    int64_t stride = h.bytes;
    switch (what) {
        case 1: h.magic ^= 1u; break;
        case 2: h.version += 1; break;
        case 3: h.bytes += 256; stride += 256; break;
        case 4: t.flags ^= STVO_SNAP_MOTION; break;
        case 5: t.cam.b += 1e-9; break;
        case 6: t.rows += 1; break;
        case 7: t.mp.min_ratio_12_l = 0.5f; break;
        case 8: t.op.max_iters_ref += 1; break;
        case 9: stride -= 16; break;
        default: break;
    }
    return snap::check_header(h, t, stride);
}

// Pack -> unpack of seeded random rows through the plain C++ statement: arrays of ONE stream cut at (K, M), counts as given, unpacked
// into arrays cut at (Kt, Mt) that were filled with 0xA5.  Returns 0 when the blob's valid rows equal the source rows, every other byte
// of the blob is zero, the unpacked rows equal the source rows, the track rows beyond the counts are zero, every other byte of the
// target is still 0xA5 and the header read back equals the one packed; a positive number says which of these failed.
int snh_roundtrip(int K, int M, int flags, int n, int nl, int kf_n, int kf_nl, int Kt, int Mt, unsigned seed) {
    stvo_snapshot_layout l;
    if (!snap::layout(K, M, flags, l)) return 100;
    const snap::Header h = header0(K, M, flags, n, nl, kf_n, kf_nl);
    unsigned long long st = 0x9E3779B97F4A7C15ull ^ seed;
    auto rnd = [&st]() { st = st * 6364136223846793005ull + 1442695040888963407ull; return (unsigned char)(st >> 56); };
    // source and target arrays sized EXACTLY to one stream's rows: a read or write outside them is the sanitizer's to find
    std::vector<std::vector<char>> src(snap::NSEC), dst(snap::NSEC);
    snap::StreamArrays a, t;
    std::memset(&a, 0, sizeof(a)); std::memset(&t, 0, sizeof(t));
    const int64_t* off = snap::offsets(l);
    for (int i = 1; i < snap::NSEC; ++i) {
        if (off[i] < 0) continue;
        const snap::SectionDef& d = snap::SECTIONS[i];
        src[i].resize((size_t)snap::cap_rows(d, K, M) * d.row_bytes);
        for (char& c : src[i]) c = (char)(rnd() | 1);  // never zero: a zero byte in the blob is a fill byte
        dst[i].assign((size_t)snap::cap_rows(d, Kt, Mt) * d.row_bytes, (char)0xA5);
        a.ptr[i] = src[i].data(); a.stride[i] = (int64_t)src[i].size();
        t.ptr[i] = dst[i].data(); t.stride[i] = (int64_t)dst[i].size();
    }
    std::vector<char> blob((size_t)l.bytes, (char)0x5A);
    snap::pack_host(l, h, a, 0, blob.data());
    std::vector<char> live((size_t)l.bytes, 0);
    for (int k = 0; k < snap::HEADER_BYTES; ++k) live[(size_t)k] = 1;
    if (std::memcmp(blob.data(), &h, sizeof(h))) return 1;
    for (int i = 1; i < snap::NSEC; ++i) {
        if (off[i] < 0) continue;
        const size_t bytes = (size_t)snap::live_rows(snap::SECTIONS[i], h) * snap::SECTIONS[i].row_bytes;
        if (bytes && std::memcmp(blob.data() + off[i], src[i].data(), bytes)) return 2;
        for (size_t k = 0; k < bytes; ++k) live[(size_t)off[i] + k] = 1;
    }
    for (size_t k = 0; k < blob.size(); ++k)
        if (!live[k] && blob[k] != 0) return 3;
    snap::Header back;
    snap::unpack_host(blob.data(), t, Kt, Mt, 0, &back);
    if (std::memcmp(&back, &h, sizeof(h))) return 4;
    for (int i = 1; i < snap::NSEC; ++i) {
        if (off[i] < 0) continue;
        const size_t bytes = (size_t)snap::live_rows(snap::SECTIONS[i], h) * snap::SECTIONS[i].row_bytes;
        if (bytes && std::memcmp(dst[i].data(), src[i].data(), bytes)) return 5;
        const bool tracks = i == snap::SEC_TRACKS_P || i == snap::SEC_TRACKS_L;
        for (size_t k = bytes; k < dst[i].size(); ++k)
            if (dst[i][k] != (tracks ? (char)0 : (char)0xA5)) return 6;
    }
    return 0;
}

// The chunk table the kernels' launch uses: returns the number of chunks (-1: none), out[0] = chunk bytes, out[1] = 1 when the chunks
// tile every present section's span exactly once, in order
int snh_chunks(int K, int M, int flags, long long* out) {
    snap::KernelArgs a;
    std::memset(&a, 0, sizeof(a));
    if (!snap::make_chunks(K, M, flags, a)) return -1;
    out[0] = a.chunk_bytes;
    int k = 0, ok = 1;
    for (int i = 0; i < snap::NSEC; ++i) {
        const snap::SectionDef& d = snap::SECTIONS[i];
        if (d.flag && !(flags & d.flag)) continue;
        int idx = 0;
        for (int64_t lo = 0; lo < snap::section_span(d, K, M); lo += a.chunk_bytes, ++idx, ++k)
            if (k >= a.n_chunks || a.chunks[k].sec != i || a.chunks[k].idx != idx) ok = 0;
    }
    out[1] = ok && k == a.n_chunks && a.chunk_bytes % 256 == 0;
    return a.n_chunks;
}

// The planner with the two facts that make the line stream wait for the step's own fork event.  facts: B, cus, frame_idx, raw_split,
// st_dirty, has_control, after_import; hist[3]; out: par, mid_fork, fork_at_start, line_forked, cells_ahead, lines_ahead, gate,
// then the eight schedule words.
void snh_plan(const int* facts, const long long* hist, int* out) {
    StepFacts f;
    f.B = facts[0]; f.K = 512; f.M = 64; f.cus = facts[1];
    f.has_points = f.has_lines = f.best_lr_matches = true;
    f.lines_now = f.lines_prev = f.track = true;
    f.frame_idx = facts[2];
    f.raw_split = facts[3]; f.raw_max_lines = 40; f.set_lines_cap_prev = f.set_lines_cap_cur = 64;
    f.st_dirty = facts[4];
    f.has_alt_m12l = f.cells_differ = f.B >= 64;
    f.grid_points_fused_ok = f.match_small_ok_K = f.match_small_ok_M = true;
    f.pose_inline_sync_ok = f.B <= 16;
    f.pose_batch_kernel_selected = f.pose_start_flag_ok = f.B >= 64;
    f.pose2p_waves_per_pair = 2;
    f.has_control = facts[5]; f.after_import = facts[6];
    StepHistory h;
    h.fork_rec_frame = hist[0]; h.pose_flag_frame = hist[1]; h.sl_forked_frame = hist[2];
    const StepPlan p = plan_step(f, h, [](int) { return true; });
    int i = 0;
    out[i++] = p.par; out[i++] = p.mid_fork; out[i++] = p.fork_at_start; out[i++] = p.line_forked;
    out[i++] = p.cells_ahead; out[i++] = p.lines_ahead; out[i++] = p.gate;
    for (int k = 0; k < 8; ++k) out[i++] = p.schedule[k];
}

}  // extern "C"
