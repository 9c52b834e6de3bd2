// The product's pipeline layouts (stvo-pl_amd/csrc/seq_layout.h, and stvo::seq_layout of seq_state.h) run on a null base, behind a flat
// C interface — TEST INFRASTRUCTURE ONLY.  tests/test_seq_layout_host.py names the entries in the same order.  Built by g++ with the
// HIP headers in host mode (-D__HIP_PLATFORM_AMD__): nothing of the runtime is called.  With SEQ_LAYOUT_HOST_MAIN it is a stand-alone
// program that walks a table of shapes (the sanitizer build).
#include <cstdio>

#include "../../stvo-pl_amd/csrc/seq_state.h"

namespace {
long long at(const void* p) { return (long long)reinterpret_cast<uintptr_t>(p); }
// a conditional buffer that was not cut: no buffer but the first raw slot sits at offset 0
long long at_opt(const void* p) { return p ? at(p) : -1; }
int put_set(const stvo::StereoSetPtrs& q, long long* out) {
    const void* p[12] = {q.rc, q.desc, q.n, q.spl, q.epl, q.sP, q.eP, q.le, q.s2l, q.s2lm, q.ldesc, q.nl};
    for (int i = 0; i < 12; ++i) out[i] = (i == 2 || i == 11) ? at_opt(p[i]) : at(p[i]);  // the counts are the conditional ones
    return 12;
}
}  // namespace

extern "C" {

// out[0..13]: the arrays of a raw slot, out[14]: first byte of the key-line part, out[15] = raw_frame_bytes; both views must agree
int slh_raw(int B, int K, int M, long long* out) {
    stvo::RawFrameSpan span;
    const stvo::RawFrame r = stvo::raw_frame<false>(nullptr, B, K, M, &span);
    const stvo::RawFrameView v = stvo::raw_frame<true>(nullptr, B, K, M);
    const void* p[14] = {r.kp_l, r.oct_l, r.desc_l, r.n_kp_l, r.kp_r, r.desc_r, r.n_kp_r, r.kl_l, r.oct_ll, r.ldesc_l, r.n_kl_l, r.kl_r, r.ldesc_r, r.n_kl_r};
    const void* q[14] = {v.kp_l, v.oct_l, v.desc_l, v.n_kp_l, v.kp_r, v.desc_r, v.n_kp_r, v.kl_l, v.oct_ll, v.ldesc_l, v.n_kl_l, v.kl_r, v.ldesc_r, v.n_kl_r};
    for (int i = 0; i < 14; ++i) {
        if (p[i] != q[i]) return -1;
        out[i] = at(p[i]);
    }
    out[14] = (long long)span.lines_off;
    out[15] = (long long)stvo::raw_frame_bytes(B, K, M);
    return span.bytes == (size_t)out[15] ? 16 : -1;
}

// the whole device allocation of a pipeline of capacity (B, K, M) with matching_s_ws = ws: out = every buffer in the order it is cut
// (tests/test_seq_layout_host.py: MAIN), then the six offsets of FetchBlock, then the total
int slh_main(int B, int K, int M, int ws, long long* out) {
    stvo_seq s;
    s.B = B; s.K = K; s.M = M;
    s.mp.matching_s_ws = ws;
    s.raw_span = stvo::raw_frame_span(B, K, M);
    const size_t total = stvo::seq_layout(s, nullptr);
    const stvo::SeqDev& d = s.d;
    const stvo_seq::CellsBuf& c1 = s.cells_buf[1];
    const bool second = c1.pstart != s.cells_buf[0].pstart;
    int n = 0;
    for (const void* p : {(const void*)s.raw_dev[0], (const void*)s.raw_dev[1], (const void*)s.d_cams, (const void*)s.d_inv_wh, (const void*)s.d_qtab,
                          (const void*)s.d_join_flag, (const void*)s.d_pose_flag, (const void*)d.pxy_l, (const void*)d.pstart, (const void*)d.pitems,
                          (const void*)d.prank, (const void*)d.pperm, (const void*)d.prange, (const void*)d.pcell})
        out[n++] = at(p);
    out[n++] = at_opt(d.plstart); out[n++] = at_opt(d.plperm);
    for (const void* p : {(const void*)c1.pstart, (const void*)c1.pperm, (const void*)c1.pcell, (const void*)c1.plstart, (const void*)c1.plperm})
        out[n++] = second ? at(p) : -1;
    for (const void* p : {(const void*)d.lxy_l, (const void*)d.lstart, (const void*)d.litems, (const void*)d.lrank, (const void*)d.lperm, (const void*)d.ldir,
                          (const void*)s.grid_p.top2, (const void*)s.grid_p.owner2, (const void*)s.grid_p.elig, (const void*)s.grid_p.elig_cnt,
                          (const void*)s.grid_p.ovf, (const void*)s.grid_l.elig, (const void*)s.grid_l.elig_cnt, (const void*)s.grid_l.ovf,
                          (const void*)s.fb.m12s_p, (const void*)s.fb.m12s_l,
                          (const void*)s.fb.m12p, (const void*)s.fb.m12l, (const void*)s.fb.inlp, (const void*)s.fb.inll, (const void*)s.results,
                          (const void*)s.counts})
        out[n++] = at(p);
    out[n++] = at_opt(s.m12l_alt);
    for (const void* p : {(const void*)s.grid_l.cover, (const void*)s.grid_l.top2, (const void*)s.grid_l.owner2, (const void*)s.lazy_l.knn12, (const void*)s.lazy_l.knn21,
                          (const void*)s.lazy_l.cand, (const void*)s.lazy_l.need, (const void*)s.lazy_l.qsel, (const void*)s.lazy_l.nsel})
        out[n++] = at(p);
    for (const stvo::StereoSetPtrs& q : s.set) n += put_set(q, out + n);
    // what SeqDev carries of the above is the same buffer
    // ... the key-points keep no bit-matrix, and misfit lies behind ovf in one buffer
    if (s.grid_p.cover != nullptr || s.grid_p.misfit != s.grid_p.ovf + B || s.grid_l.misfit != nullptr) return -1;
    if (d.cams != s.d_cams || d.inv_wh != s.d_inv_wh || d.top2_p != s.grid_p.top2 || d.govf_p != s.grid_p.ovf || d.m12s_p != s.fb.m12s_p || d.m12s_l != s.fb.m12s_l ||
        s.cells_buf[0].pstart != d.pstart || s.cells_buf[0].plperm != d.plperm || s.lazy_l.knn_capacity != (size_t)B * M * 4)
        return -1;
    for (size_t o : {s.fb.off_m12s_l, s.fb.off_m12p, s.fb.off_m12l, s.fb.off_inlp, s.fb.off_inll, s.fb.off_flag}) out[n++] = (long long)o;
    out[n++] = (long long)s.fb.m12_span();
    out[n++] = (long long)s.fb.inl_span();
    out[n++] = (long long)total;
    return n;
}

// a key-frame set as stvo_seq_set_tracks cuts it: the twelve entries of the set (counts absent), the headers, the total
int slh_keyframe(int B, int K, int M, long long* out) {
    stvo::Carver c(nullptr);
    const stvo::StereoSetPtrs q = stvo::carve_stereo_set(c, B, K, M, false);
    int n = put_set(q, out);
    out[n++] = at(c.take<stvo_kf_header>((size_t)B));
    out[n++] = (long long)c.off;
    return n;
}
}

#ifdef SEQ_LAYOUT_HOST_MAIN
int main() {
    static const int shapes[][4] = {{1, 64, 64, 10},     {1, 2048, 320, 10},  {16, 1024, 128, 10}, {17, 1024, 128, 10},  {63, 512, 128, 10},
                                    {64, 512, 128, 10},  {2, 2048, 512, 16},  {2, 2048, 512, 17},  {2, 2048, 512, -1},   {64, 2048, 512, 0},
                                    {3072, 1024, 128, 10}};
    long long out[160];
    for (const auto& sh : shapes) {
        const int a = slh_raw(sh[0], sh[1], sh[2], out), b = slh_main(sh[0], sh[1], sh[2], sh[3], out);
        const long long total = b > 0 ? out[b - 1] : 0;
        const int c = slh_keyframe(sh[0], sh[1], sh[2], out);
        if (a < 0 || b < 0 || c < 0) {
            std::printf("layout inconsistent at B %d K %d M %d ws %d\n", sh[0], sh[1], sh[2], sh[3]);
            return 1;
        }
        std::printf("B %4d K %4d M %3d ws %2d: %d + %d + %d entries, %lld bytes\n", sh[0], sh[1], sh[2], sh[3], a, b, c, total);
    }
    return 0;
}
#endif
