// stream_snapshot.hip — the two kernels behind stvo_seq_export_streams / stvo_seq_import_streams (seq_snapshot.hip): a stream's state
// between two steps into one blob, and a blob into a stream.  The layout, the header and the argument block: stream_snapshot.h.
//   snapshot_pack_kernel     blob <- rows [0, count) of every section of the stream, the header, and zero for every other byte
//   snapshot_unpack_kernel   stream <- rows [0, count) of every section of the blob, the counts and the key-frame header; the track
//                            state's rows beyond the counts become zero
// One launch covers every blob of a call and every section: grid (chunk of a section, blob).  A workgroup reads its stream's counts
// (uniform loads: no broadcast, no barrier), derives its byte range and moves it in 16-byte words with four loads in flight per lane
// (copy_words.h), the odd 8-byte word of a range by one lane.  Every offset in a blob is a multiple of 256 and every row a multiple
// of 8 bytes; the one array whose per-stream stride is no multiple of 16 (stvo_traj_state, 856 bytes) moves in 8-byte words.  Plain
// vector loads and stores, no atomics, no LDS.
#include "copy_words.h"
#include "ctx_internal.h"
#include "stream_snapshot.h"

namespace stvo {
namespace {

constexpr int SNAP_BLOCK = 256;
typedef unsigned long long u64;

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
__device__ __forceinline__ int64_t lo_of(int64_t x, int64_t y) { return x < y ? x : y; }
__device__ __forceinline__ int64_t hi_of(int64_t x, int64_t y) { return x > y ? x : y; }

// bytes [lo, hi) of src to the same bytes of dst; lo, hi multiples of 8.  wide: src + lo and dst + lo are 16-byte aligned.
__device__ __forceinline__ void copy_range(const char* __restrict__ src, char* __restrict__ dst, int64_t lo, int64_t hi, bool wide, int tid) {
    if (hi <= lo) return;
    const int64_t len = hi - lo;
    if (!wide) {
        copy_words<u64, SNAP_BLOCK>(src + lo, dst + lo, 0, (int)(len >> 3), tid);
        return;
    }
    const int n16 = (int)(len >> 4);
    copy_words<uint4, SNAP_BLOCK>(src + lo, dst + lo, 0, n16, tid);
    if ((len & 8) && tid == 0) *reinterpret_cast<u64*>(dst + lo + ((int64_t)n16 << 4)) = *reinterpret_cast<const u64*>(src + lo + ((int64_t)n16 << 4));
}

// bytes [lo, hi) of dst become zero; lo a multiple of 8, hi of 16, dst 16-byte aligned
__device__ __forceinline__ void zero_range(char* __restrict__ dst, int64_t lo, int64_t hi, int tid) {
    if (hi <= lo) return;
    if (lo & 8) {
        if (tid == 0) *reinterpret_cast<u64*>(dst + lo) = 0ull;
        lo += 8;
    }
    fill_words<uint4, SNAP_BLOCK>(dst + lo, 0, (int)((hi - lo) >> 4), make_uint4(0u, 0u, 0u, 0u), tid);
}

__global__ __launch_bounds__(SNAP_BLOCK) void snapshot_pack_kernel(snap::KernelArgs a) {
    const int tid = threadIdx.x, blob_i = blockIdx.y;
    const snap::Chunk ch = a.chunks[blockIdx.x];
    const int b = a.streams[2 * blob_i];
    char* blob = a.blobs + (int64_t)blob_i * a.blob_stride;
    const stvo_snapshot_layout& l = a.lay[0];
    const stvo_kf_header kf = a.kf_hdr ? a.kf_hdr[b] : stvo_kf_header{0, 0, 0, 0};
    const int n = clampi(a.n[b], a.K), nl = clampi(a.nl[b], a.M), kf_n = clampi(kf.n_pts, a.K), kf_nl = clampi(kf.n_lines, a.M);
    if (ch.sec == snap::SEC_HEADER) {
        if (tid != 0) return;
        // (the record has no padding: every byte of the section is written)
        snap::Header* h = reinterpret_cast<snap::Header*>(blob + l.off_header);
        h->magic = snap::MAGIC; h->version = snap::VERSION; h->bytes = l.bytes;
        h->K = l.K; h->M = l.M; h->flags = l.flags; h->n = n; h->nl = nl; h->reserved = 0;
        h->kf = stvo_kf_header{kf_n, kf_nl, kf.frame, kf.serial};
        h->cam = a.cams[b];
        h->cols = a.img_size[2 * b]; h->rows = a.img_size[2 * b + 1];
        h->mp = a.mp; h->op = a.op;
        return;
    }
    const snap::SectionDef d = a.sec[ch.sec];
    const int64_t off = snap::offsets(l)[ch.sec];
    const int64_t span = snap::section_span(d, l.K, l.M), lo = (int64_t)ch.idx * a.chunk_bytes;
    if (off < 0 || lo >= span) return;
    const int64_t hi = lo_of(lo + a.chunk_bytes, span), live = (int64_t)snap::live_rows(d, n, nl, kf_n, kf_nl) * d.row_bytes;
    const char* src = a.arr.ptr[ch.sec] + (int64_t)b * a.arr.stride[ch.sec];
    copy_range(src, blob + off, lo, lo_of(hi, live), (a.arr.stride[ch.sec] & 15) == 0, tid);
    zero_range(blob + off, hi_of(lo, live), hi, tid);
}

__global__ __launch_bounds__(SNAP_BLOCK) void snapshot_unpack_kernel(snap::KernelArgs a) {
    const int tid = threadIdx.x, blob_i = blockIdx.y;
    const snap::Chunk ch = a.chunks[blockIdx.x];
    const int b = a.streams[2 * blob_i];
    const stvo_snapshot_layout& l = a.lay[a.streams[2 * blob_i + 1]];
    const char* blob = a.blobs + (int64_t)blob_i * a.blob_stride;
    // (the host has checked these against both capacities; the clamps keep a blob that changed since inside the stream's rows)
    const snap::Header* h = reinterpret_cast<const snap::Header*>(blob + l.off_header);
    const stvo_kf_header kf = h->kf;
    const int capK = a.K < l.K ? a.K : l.K, capM = a.M < l.M ? a.M : l.M;
    const int n = clampi(h->n, capK), nl = clampi(h->nl, capM), kf_n = clampi(kf.n_pts, capK), kf_nl = clampi(kf.n_lines, capM);
    if (ch.sec == snap::SEC_HEADER) {
        if (tid != 0) return;
        a.n[b] = n;
        a.nl[b] = nl;
        if (a.kf_hdr) *reinterpret_cast<int4*>(a.kf_hdr + b) = make_int4(kf_n, kf_nl, kf.frame, kf.serial);
        return;
    }
    const snap::SectionDef d = a.sec[ch.sec];
    const int64_t off = snap::offsets(l)[ch.sec];
    const int64_t span = snap::section_span(d, l.K, l.M), lo = (int64_t)ch.idx * a.chunk_bytes;
    if (off < 0 || lo >= span) return;
    const int64_t hi = lo_of(lo + a.chunk_bytes, span), live = (int64_t)snap::live_rows(d, n, nl, kf_n, kf_nl) * d.row_bytes;
    char* dst = a.arr.ptr[ch.sec] + (int64_t)b * a.arr.stride[ch.sec];
    copy_range(blob + off, dst, lo, lo_of(hi, live), (a.arr.stride[ch.sec] & 15) == 0, tid);
    if (ch.sec == snap::SEC_TRACKS_P || ch.sec == snap::SEC_TRACKS_L) {
        // the stream's rows beyond the count, up to ITS capacity: the section's last chunk takes what lies beyond the blob's span
        const int64_t dst_bytes = snap::cap_rows(d, a.K, a.M) * d.row_bytes;
        zero_range(dst, hi_of(lo, live), hi == span ? dst_bytes : lo_of(hi, dst_bytes), tid);
    }
}

static_assert(sizeof(stvo_kf_header) == sizeof(int4), "the key-frame header is stored as one 16-byte word");
static_assert(sizeof(snap::KernelArgs) <= 4096, "the argument block travels by value");

}  // namespace

void launch_snapshot_pack(hipStream_t s, const snap::KernelArgs& a) {
    hipLaunchKernelGGL(snapshot_pack_kernel, dim3(a.n_chunks, a.n_blobs), dim3(SNAP_BLOCK), 0, s, a);
}

void launch_snapshot_unpack(hipStream_t s, const snap::KernelArgs& a) {
    hipLaunchKernelGGL(snapshot_unpack_kernel, dim3(a.n_chunks, a.n_blobs), dim3(SNAP_BLOCK), 0, s, a);
}

}  // namespace stvo
