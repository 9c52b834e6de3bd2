// stream_snapshot.h — the snapshot of ONE stream of the device-resident pipeline (stvo_seq_export_streams / stvo_seq_import_streams):
// the blob's layout, its header, the check an import makes of a header, and the argument block of the two kernels
// (stream_snapshot.hip), each stated ONCE.  Host-pure like seq_layout.h (g++ alone compiles it): tests/cpp/snapshot_host.cpp runs the
// layout, the check and a plain C++ pack / unpack (below) without a device.
//
// A blob is cut with the Carver at the EXPORTING pipeline's capacities K, M and feature flags: every section starts 256-aligned at an
// offset that depends on (K, M, flags) alone, a section of a feature that is off is not cut, and every byte that is no valid row and no
// header field is zero — a blob is a function of the state.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../include/stvo_hip.h"
#include "seq_layout.h"

#if defined(__HIPCC__)
#define STVO_SNAP_HD __host__ __device__ __forceinline__
#else
#define STVO_SNAP_HD inline
#endif

namespace stvo {
namespace snap {

constexpr uint32_t MAGIC = 0x53567453u;  // "StVS"
constexpr uint32_t VERSION = 1;

constexpr int FLAGS_ALL = STVO_SNAP_MOTION | STVO_SNAP_TRAJ | STVO_SNAP_TRAJ_KF | STVO_SNAP_TRACKS | STVO_SNAP_KF_SETS;
// key-frames need the trajectory, key-frame sets need the tracks
inline bool flags_legal(int f) {
    return (f & ~FLAGS_ALL) == 0 && (!(f & STVO_SNAP_TRAJ_KF) || (f & STVO_SNAP_TRAJ)) && (!(f & STVO_SNAP_KF_SETS) || (f & STVO_SNAP_TRACKS));
}

// ---- the sections, in the order they are cut ---------------------------------------------------------------------------------------
// rows: what bounds the section (K rows, M rows, or one record); count: which count of the stream says how many rows are live.
enum Rows : int32_t { ROWS_ONE = 0, ROWS_K = 1, ROWS_M = 2 };
enum Count : int32_t { COUNT_ONE = 0, COUNT_N = 1, COUNT_NL = 2, COUNT_KF_N = 3, COUNT_KF_NL = 4 };
struct SectionDef {
    int32_t row_bytes, rows, count, flag;  // flag: the feature the section belongs to (0: always there)
};
constexpr int SEC_HEADER = 0, SEC_SET = 1, SEC_MOTION = 11, SEC_TRAJ = 12, SEC_TRACKS_P = 13, SEC_TRACKS_L = 14, SEC_KF = 15, NSEC = 25;
constexpr int HEADER_BYTES = 256, D = (int)sizeof(double);
#define STVO_SNAP_SET_SECTIONS(cn, cnl, fl)                                                                              \
    {(int)sizeof(float4), ROWS_K, cn, fl}, {STVO_DESC_BYTES, ROWS_K, cn, fl}, {2 * D, ROWS_M, cnl, fl}, {2 * D, ROWS_M, cnl, fl},    \
    {3 * D, ROWS_M, cnl, fl}, {3 * D, ROWS_M, cnl, fl}, {3 * D, ROWS_M, cnl, fl}, {D, ROWS_M, cnl, fl}, {D, ROWS_M, cnl, fl},         \
    {STVO_DESC_BYTES, ROWS_M, cnl, fl}
// (the arrays of a stereo set in the order of StereoSetPtrs: rc, desc, spl, epl, sP, eP, le, s2l, s2lm, ldesc)
constexpr SectionDef SECTIONS[NSEC] = {
    {HEADER_BYTES, ROWS_ONE, COUNT_ONE, 0},
    STVO_SNAP_SET_SECTIONS(COUNT_N, COUNT_NL, 0),
    {16 * D, ROWS_ONE, COUNT_ONE, STVO_SNAP_MOTION},
    {(int)sizeof(stvo_traj_state), ROWS_ONE, COUNT_ONE, STVO_SNAP_TRAJ},
    {(int)sizeof(stvo_track), ROWS_K, COUNT_N, STVO_SNAP_TRACKS},
    {(int)sizeof(stvo_track), ROWS_M, COUNT_NL, STVO_SNAP_TRACKS},
    STVO_SNAP_SET_SECTIONS(COUNT_KF_N, COUNT_KF_NL, STVO_SNAP_KF_SETS),
};
#undef STVO_SNAP_SET_SECTIONS
static_assert(sizeof(stvo_traj_state) % 8 == 0 && sizeof(stvo_track) == 8, "every row is a whole number of 8-byte words");

STVO_SNAP_HD int64_t cap_rows(const SectionDef& d, int K, int M) { return d.rows == ROWS_K ? K : (d.rows == ROWS_M ? M : 1); }

// The public layout record holds `bytes` and then one offset per section, in the order of SECTIONS.
static_assert(offsetof(stvo_snapshot_layout, off_header) == 8 && offsetof(stvo_snapshot_layout, off_kf_ldesc) == 8 * NSEC &&
              offsetof(stvo_snapshot_layout, K) == 8 * (NSEC + 1), "stvo_snapshot_layout lists the sections in the order they are cut");
STVO_SNAP_HD const int64_t* offsets(const stvo_snapshot_layout& l) { return &l.off_header; }
STVO_SNAP_HD int64_t* offsets(stvo_snapshot_layout& l) { return &l.off_header; }

// The one statement of the layout.  An absent section has offset -1.
inline bool layout(int K, int M, int flags, stvo_snapshot_layout& l) {
    if (K <= 0 || M <= 0 || !flags_legal(flags)) return false;
    Carver c(nullptr);
    int64_t* off = offsets(l);
    for (int i = 0; i < NSEC; ++i) {
        const SectionDef& d = SECTIONS[i];
        const bool there = d.flag == 0 || (flags & d.flag);
        off[i] = there ? (int64_t) reinterpret_cast<uintptr_t>(c.take<char>((size_t)cap_rows(d, K, M) * d.row_bytes)) : -1;
    }
    l.bytes = (int64_t)c.off;
    l.K = K; l.M = M; l.flags = flags; l.reserved = 0;
    return true;
}
// bytes a present section occupies in the blob: up to where the next cut begins
STVO_SNAP_HD int64_t section_span(const SectionDef& d, int K, int M) { return ((int64_t)cap_rows(d, K, M) * d.row_bytes + 255) & ~int64_t(255); }

// ---- the header section ------------------------------------------------------------------------------------------------------------
struct Header {
    uint32_t magic, version;
    int64_t bytes;                // of the whole blob
    int32_t K, M, flags;          // of the exporting pipeline
    int32_t n, nl;                // valid rows of the stereo set
    int32_t reserved;
    stvo_kf_header kf;            // all-zero without key-frame sets; `frame` names a step of the EXPORTING pipeline
    stvo_cam cam;                 // the stream's calibration and image size
    int32_t cols, rows;
    stvo_match_params mp;         // the pipeline's parameters, byte for byte
    stvo_opt_params op;
};
static_assert(sizeof(Header) == HEADER_BYTES, "the header fills its section: no byte of it is padding");

// What one stream of the importing pipeline asks of a blob.
struct Target {
    int K, M, flags;
    stvo_cam cam;
    int32_t cols, rows;
    stvo_match_params mp;
    stvo_opt_params op;
};

// The refusals of an import, decided from the header alone (include/stvo_hip.h has the table).  blob_stride: bytes the caller says lie
// between two blobs.
inline int check_header(const Header& h, const Target& t, int64_t blob_stride) {
    if (h.magic != MAGIC || h.version != VERSION) return STVO_ERR_INVALID_ARG;
    stvo_snapshot_layout l;
    if (!layout(h.K, h.M, h.flags, l) || h.bytes != l.bytes || blob_stride < l.bytes) return STVO_ERR_INVALID_ARG;
    if (h.flags != t.flags) return STVO_ERR_INVALID_ARG;
    if (std::memcmp(&h.cam, &t.cam, sizeof(stvo_cam)) != 0 || h.cols != t.cols || h.rows != t.rows) return STVO_ERR_INVALID_ARG;
    if (std::memcmp(&h.mp, &t.mp, sizeof(stvo_match_params)) != 0 || std::memcmp(&h.op, &t.op, sizeof(stvo_opt_params)) != 0) return STVO_ERR_INVALID_ARG;
    // counts no exporter writes
    if (h.n < 0 || h.n > h.K || h.nl < 0 || h.nl > h.M || h.kf.n_pts < 0 || h.kf.n_pts > h.K || h.kf.n_lines < 0 || h.kf.n_lines > h.M)
        return STVO_ERR_INVALID_ARG;
    if (!(h.flags & STVO_SNAP_KF_SETS) && (h.kf.n_pts | h.kf.n_lines | h.kf.frame | h.kf.serial)) return STVO_ERR_INVALID_ARG;
    if (h.n > t.K || h.nl > t.M || h.kf.n_pts > t.K || h.kf.n_lines > t.M) return STVO_ERR_CAPACITY;
    return STVO_OK;
}

STVO_SNAP_HD int32_t live_rows(const SectionDef& d, int32_t n, int32_t nl, int32_t kf_n, int32_t kf_nl) {
    return d.count == COUNT_N ? n : d.count == COUNT_NL ? nl : d.count == COUNT_KF_N ? kf_n : d.count == COUNT_KF_NL ? kf_nl : 1;
}
STVO_SNAP_HD int32_t live_rows(const SectionDef& d, const Header& h) { return live_rows(d, h.n, h.nl, h.kf.n_pts, h.kf.n_lines); }

// ---- one stream's arrays in a pipeline, section by section ------------------------------------------------------------------------------
// ptr[i]: the first row of stream 0 of section i (nullptr: absent; the header has none), stride[i]: bytes from one stream to the next.
struct StreamArrays {
    char* ptr[NSEC];
    int64_t stride[NSEC];
};

// ---- plain C++ pack / unpack: the statement the kernels are held to (tests/cpp/snapshot_host.cpp) -------------------------------------------
// `h` carries the counts and every header field; arrays of stream b; blob: l.bytes bytes.
inline void pack_host(const stvo_snapshot_layout& l, const Header& h, const StreamArrays& a, int b, char* blob) {
    std::memset(blob, 0, (size_t)l.bytes);
    std::memcpy(blob + l.off_header, &h, sizeof(h));
    const int64_t* off = offsets(l);
    for (int i = 1; i < NSEC; ++i)
        if (off[i] >= 0) std::memcpy(blob + off[i], a.ptr[i] + (int64_t)b * a.stride[i], (size_t)live_rows(SECTIONS[i], h) * SECTIONS[i].row_bytes);
}
// The rows of the blob into stream b of arrays cut at other capacities (the caller has checked the header).  The track rows beyond the
// counts become zero, which is what a pipeline's first step finds there; rows of the sets beyond the counts stay.
inline void unpack_host(const char* blob, const StreamArrays& a, int K_dst, int M_dst, int b, Header* h_out) {
    Header h;
    std::memcpy(&h, blob, sizeof(h));
    stvo_snapshot_layout l;
    layout(h.K, h.M, h.flags, l);
    const int64_t* off = offsets(l);
    for (int i = 1; i < NSEC; ++i) {
        if (off[i] < 0) continue;
        const SectionDef& d = SECTIONS[i];
        char* dst = a.ptr[i] + (int64_t)b * a.stride[i];
        const size_t live = (size_t)live_rows(d, h) * d.row_bytes;
        std::memcpy(dst, blob + off[i], live);
        if (i == SEC_TRACKS_P || i == SEC_TRACKS_L) std::memset(dst + live, 0, (size_t)cap_rows(d, K_dst, M_dst) * d.row_bytes - live);
    }
    if (h_out) *h_out = h;
}

// ---- the kernels' argument block --------------------------------------------------------------------------------------------------------
// A launch covers n blobs x every chunk of every section.  A chunk is up to `chunk_bytes` of one section's span; the table is built from
// the largest capacities among the call's layouts, a workgroup whose chunk begins beyond its own blob's section leaves.
constexpr int MAX_CHUNKS = 96, MAX_LAYOUTS = 4;
struct Chunk {
    uint16_t sec, idx;
};
struct KernelArgs {
    int n_blobs;
    int K, M;                        // the pipeline's capacities
    int n_chunks;
    int64_t chunk_bytes;             // a multiple of 256
    Chunk chunks[MAX_CHUNKS];
    SectionDef sec[NSEC];            // SECTIONS, where the kernels can index it
    stvo_snapshot_layout lay[MAX_LAYOUTS];  // export: lay[0] alone.  import: the distinct layouts of the call's blobs
    const int32_t* streams;          // [n_blobs][2] device: stream of the pipeline, index into lay
    char* blobs;
    int64_t blob_stride;
    StreamArrays arr;
    int32_t *n, *nl;                 // [B] counts of the stereo set
    stvo_kf_header* kf_hdr;          // [B] or nullptr
    // what the pack kernel writes into the header besides the counts
    const stvo_cam* cams;            // [B]
    const int32_t* img_size;         // [B][2] cols, rows
    stvo_match_params mp;
    stvo_opt_params op;
};

// The chunk table for sections cut at capacities (K, M) with `flags`; false: more chunks than the table holds (never at the capacities
// a pipeline accepts).
inline bool make_chunks(int K, int M, int flags, KernelArgs& a) {
    for (int64_t cb = 16 << 10;; cb *= 2) {
        int n = 0;
        bool fits = true;
        for (int i = 0; i < NSEC && fits; ++i) {
            const SectionDef& d = SECTIONS[i];
            if (d.flag && !(flags & d.flag)) continue;
            const int64_t span = section_span(d, K, M);
            for (int64_t lo = 0, k = 0; lo < span; lo += cb, ++k) {
                if (n == MAX_CHUNKS) { fits = false; break; }
                a.chunks[n++] = Chunk{(uint16_t)i, (uint16_t)k};
            }
        }
        if (fits) {
            for (int i = 0; i < NSEC; ++i) a.sec[i] = SECTIONS[i];
            a.n_chunks = n;
            a.chunk_bytes = cb;
            return true;
        }
        if (cb > (int64_t(1) << 30)) return false;
    }
}

}  // namespace snap
}  // namespace stvo
