// seq_debug.hip — the test hooks of the device-resident pipeline (seq_pipeline.hip) and its live stage timing: entry points that look at
// what the last step left and change nothing a later step reads.  State and layout: seq_state.h.
#include <algorithm>

#include "seq_state.h"

extern "C" {

int stvo_seq_set_stage_timing(stvo_seq* s, int enable) {
    if (!s) return STVO_ERR_INVALID_ARG;
    s->timing = enable == 2 ? 2 : (enable != 0);
    s->tev_used = 0;
    return STVO_OK;
}

int stvo_seq_get_stage_timing(stvo_seq* s, float avg_ms[STVO_SEQ_NSTAGE], int32_t* n_steps) {
    if (!s || !avg_ms || !n_steps) return STVO_ERR_INVALID_ARG;
    stvo_ctx* ctx = s->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    double acc[STVO_SEQ_NSTAGE] = {0};
    int cnt[STVO_SEQ_NSTAGE] = {0};
    for (size_t k = 0; k + 2 * STVO_SEQ_NSTAGE <= s->tev_used; k += 2 * STVO_SEQ_NSTAGE)
        for (int st = 0; st < STVO_SEQ_NSTAGE; ++st) {
            if (s->timing == 2 && (st == 0 || st == 3)) continue;  // light: these pairs were not recorded (their events may hold older stamps)
            float ms = 0.f;  // a stage that did not run in this step (first frame: no f2f, no pose) left its events unrecorded
            if (hipEventElapsedTime(&ms, s->tev[k + 2 * st], s->tev[k + 2 * st + 1]) == hipSuccess) {
                acc[st] += ms;
                ++cnt[st];
            }
        }
    (void)hipGetLastError();  // unrecorded events report an error that is not one
    int n = 0;
    for (int st = 0; st < STVO_SEQ_NSTAGE; ++st) {
        avg_ms[st] = cnt[st] ? (float)(acc[st] / cnt[st]) : 0.f;
        if (cnt[st] > n) n = cnt[st];
    }
    *n_steps = n;
    s->tev_used = 0;
    return STVO_OK;
}

// TEST HOOK.  The grid structures the LAST step built on the device for sequence b: the CSR bucket grid of the right
// features (point_cells_kernel / line_cells_kernel: GridStructure + LineIterator of the reference), the integer cells of
// the left features, and — decoded from grid_cover's bit matrix — the candidate set GridStructure::get returned for every
// left feature.  tests/test_gpu_grid_ref.py compares them cell for cell with outputs of the reference's own
// gridStructure.cpp / lineIterator.cpp (tests/golden/ref_device_grid_goldens.npz).
int stvo_seq_debug_grid(stvo_seq* s, int b, int lines, int32_t* cell_start, int32_t* cell_items, int32_t cap_items,
                        int32_t* cells_left, int32_t* cand_off, int32_t* cand, int32_t cap_cand, int32_t* n_left_out) {
    if (!s || b < 0 || b >= s->B || !cell_start || !cell_items || !cells_left || !cand_off || !cand || !n_left_out || s->frame_idx == 0)
        return STVO_ERR_INVALID_ARG;
    stvo_ctx* ctx = s->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(s->line_stream));
    const stvo::SeqDev& d = s->d;
    stvo::SeqDev full = d;
    full.raw = s->raw_view(s->last_slot);
    if (!lines && s->last_point_lean) {  // the step ran the lean cells kernel: produce the full set of grid arrays for the hook
        stvo::launch_point_cells(ctx->stream, full, false);
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    if (lines && s->last_line_fused) {  // the step ran the fused line kernel: the general matcher's kernels produce the grid arrays
        stvo::launch_line_cells(ctx->stream, full);
        stvo::launch_grid_batch(ctx->stream, stvo::line_grid_args(s, full));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    const int R = lines ? s->M : s->K, xyw = lines ? 4 : 2;
    const size_t items_stride = lines ? (size_t)s->M * stvo::LENT : (size_t)s->K;
    // counts of the slot the last step ran on are not tracked per slot: read them through the last bound raw block
    int32_t nl = 0, nr = 0;
    HIP_TRY(ctx, hipMemcpy(&nl, (lines ? full.raw.n_kl_l : full.raw.n_kp_l) + b, 4, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(&nr, (lines ? full.raw.n_kl_r : full.raw.n_kp_r) + b, 4, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(cell_start, (lines ? d.lstart : d.pstart) + (size_t)b * (STVO_GRID_CELLS + 1),
                           (STVO_GRID_CELLS + 1) * sizeof(int32_t), hipMemcpyDeviceToHost));
    const int n_items = cell_start[STVO_GRID_CELLS];
    if (n_items < 0 || (size_t)n_items > items_stride) return STVO_ERR_HIP;
    if (n_items > cap_items) return STVO_ERR_CAPACITY;
    if (n_items) HIP_TRY(ctx, hipMemcpy(cell_items, (lines ? d.litems : d.pitems) + (size_t)b * items_stride, (size_t)n_items * 4, hipMemcpyDeviceToHost));
    if (nl) HIP_TRY(ctx, hipMemcpy(cells_left, (lines ? d.lxy_l : d.pxy_l) + (size_t)b * R * xyw, (size_t)nl * xyw * 4, hipMemcpyDeviceToHost));
    // candidate sets: bit p % 64 of cover[p / 64][i1] <=> right feature perm[p] is a candidate of left feature i1
    const stvo::GridMatrixDims md = stvo::grid_matrix_dims(R, R);
    const int words64 = md.words64;
    std::vector<unsigned long long> cover(md.words());  // (no key-point stage: no candidates)
    std::vector<int32_t> perm((size_t)R);
    if (lines) {
        HIP_TRY(ctx, hipMemcpy(cover.data(), s->grid_l.cover + (size_t)b * cover.size(), cover.size() * 8, hipMemcpyDeviceToHost));
    } else if (s->op.has_points) {
        // the point matchers derive their masks from ranges and the pipeline keeps no key-point matrix: materialise exactly those masks
        // for frame b, in a matrix that lives for this call
        stvo::GridMatch g = stvo::point_grid_args(s, full);
        HIP_TRY(ctx, hipMalloc((void**)&g.s.cover, cover.size() * 8));
        stvo::launch_grid_range_debug(ctx->stream, g, b);
        hipError_t e = hipStreamSynchronize(ctx->stream);
        if (e == hipSuccess) e = hipMemcpy(cover.data(), g.s.cover, cover.size() * 8, hipMemcpyDeviceToHost);
        (void)hipFree(g.s.cover);
        HIP_TRY(ctx, e);
    }
    HIP_TRY(ctx, hipMemcpy(perm.data(), (lines ? d.lperm : d.pperm) + (size_t)b * R, perm.size() * 4, hipMemcpyDeviceToHost));
    int tot = 0;
    std::vector<int32_t> row;
    for (int i1 = 0; i1 < nl; ++i1) {
        row.clear();
        for (int w = 0; w < words64; ++w) {
            unsigned long long m = cover[(size_t)w * R + i1];
            while (m) {
                const int p = w * 64 + __builtin_ctzll(m);
                m &= m - 1ull;
                if (p < nr) row.push_back(perm[p]);
            }
        }
        std::sort(row.begin(), row.end());
        cand_off[i1] = tot;
        for (int id : row) {
            if (tot < cap_cand) cand[tot] = id;
            ++tot;
        }
    }
    cand_off[nl] = tot;
    *n_left_out = nl;
    return tot > cap_cand ? STVO_ERR_CAPACITY : STVO_OK;
}

// TEST HOOK.  Which way the stereo point matcher of the LAST step took each frame: out[b] = {misfit, ovf}, the two words the matcher keeps
// side by side (GridScratch: ovf[B] then misfit[B]).  Copies only: nothing is launched, no state of `s` changes.  A word that the route of
// the step did not write for a frame is reported as 0, not as an earlier step left it: misfit belongs to the one-workgroup kernel
// (lean_cells), ovf to a frame the scan formulation ran with best_lr_matches on (every frame of the scan route, the misfit frames of
// the other).  Ask BEFORE stvo_seq_debug_grid: after a step of the one-workgroup route that hook runs the full cells kernel, which
// clears ovf.
int stvo_seq_debug_point_route(stvo_seq* s, int32_t* out) {
    if (!s || !out || s->frame_idx == 0) return STVO_ERR_INVALID_ARG;
    stvo_ctx* ctx = s->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(s->line_stream));
    const int B = s->B;
    std::vector<int32_t> w(stvo::grid_route_words(B), 0);  // ovf[B] then misfit[B], ONE buffer (grid_scratch.h)
    if (s->op.has_points) HIP_TRY(ctx, hipMemcpy(w.data(), s->grid_p.ovf, w.size() * 4, hipMemcpyDeviceToHost));
    const bool fused = s->op.has_points && s->last_point_lean, lr = s->last_mutual;
    for (int b = 0; b < B; ++b) {
        const int misfit = fused ? w[(size_t)B + b] : 0;
        const bool scanned = s->op.has_points && (!fused || misfit != 0);
        out[2 * b] = misfit;
        out[2 * b + 1] = scanned && lr ? w[b] : 0;
    }
    return STVO_OK;
}

// TEST HOOK.  The stereo sets the LAST step built from its frame for sequence b, as the tails of the association left them
// (point_tail.h / fused_tail; line_tail_frame): tests/test_gpu_stereo_tail.py compares them record by record with the oracle and
// with tests/np_stereo_tail.py.  Copies only: nothing is launched, no state of `s` changes.
// Which of the three sets: every step — whatever its schedule, the key-line stage ahead included, which only moves the key-line
// kernels of a step behind an earlier event — writes set[cur] and then advances cur, so the last step's set is set[prev_set()] (what
// stvo_seq_read reads its counts from).  Before the first step no set belongs to a frame: STVO_ERR_INVALID_ARG.
int stvo_seq_debug_stereo(stvo_seq* s, int b, int32_t cap_pts, int32_t* n_pts, float* rc, uint8_t* desc, int32_t cap_lines,
                          int32_t* n_lines, double* spl, double* epl, double* sP, double* eP, double* le, double* s2l, double* s2lm,
                          uint8_t* ldesc) {
    if (!s || b < 0 || b >= s->B || cap_pts < 0 || cap_lines < 0 || !n_pts || !n_lines || s->frame_idx == 0) return STVO_ERR_INVALID_ARG;
    if ((cap_pts > 0 && (!rc || !desc)) || (cap_lines > 0 && (!spl || !epl || !sP || !eP || !le || !s2l || !s2lm || !ldesc)))
        return STVO_ERR_INVALID_ARG;
    stvo_ctx* ctx = s->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(s->line_stream));
    const stvo::StereoSetPtrs& ls = s->set[s->prev_set()];
    const size_t K = (size_t)s->K, M = (size_t)s->M;
    int32_t n = 0, nl = 0;
    if (s->op.has_points) HIP_TRY(ctx, hipMemcpy(&n, ls.n + b, 4, hipMemcpyDeviceToHost));
    if (s->last_lines) HIP_TRY(ctx, hipMemcpy(&nl, ls.nl + b, 4, hipMemcpyDeviceToHost));
    if (n < 0 || (size_t)n > K || nl < 0 || (size_t)nl > M) return STVO_ERR_HIP;
    *n_pts = n;
    *n_lines = nl;
    if (n > cap_pts || nl > cap_lines) return STVO_ERR_CAPACITY;
    return stvo::copy_out_stereo_set(ctx, ls, b, K, M, n, nl,
                                     stvo::StereoSetPtrs{reinterpret_cast<float4*>(rc), desc, nullptr, spl, epl, sP, eP, le, s2l, s2lm, ldesc, nullptr});
}

}  // extern "C"
