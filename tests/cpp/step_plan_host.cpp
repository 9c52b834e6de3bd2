// The product's step planner (stvo-pl_amd/csrc/step_plan.h) compiled for the host, behind a flat C interface — TEST INFRASTRUCTURE ONLY.
// tests/step_plan_host_lib.py names the entries of the three arrays in the same order.
#include "../../stvo-pl_amd/csrc/step_plan.h"

extern "C" {

// facts[29], sw[9] (INT_MIN: unset), hist[3] (in; out when do_commit), lds_fits: the fake answer of the LDS opt-in;
// out[46]: the plan's fields, its schedule record, how often the opt-in was asked and for how many bytes
void sph_plan(const int* facts, const int* sw, long long* hist, int lds_fits, int do_commit, int* out) {
    stvo::StepFacts f;
    int i = 0;
    f.B = facts[i++]; f.K = facts[i++]; f.M = facts[i++]; f.cus = facts[i++];
    f.has_points = facts[i++]; f.has_lines = facts[i++]; f.best_lr_matches = facts[i++];
    f.lines_now = facts[i++]; f.lines_prev = facts[i++]; f.track = facts[i++];
    f.frame_idx = facts[i++];
    f.raw_split = facts[i++]; f.raw_max_lines = facts[i++]; f.set_lines_cap_prev = facts[i++]; f.set_lines_cap_cur = facts[i++];
    f.st_dirty = facts[i++]; f.fetch = facts[i++]; f.zero_copy = facts[i++];
    f.timing = facts[i++]; f.timing_events = facts[i++];
    f.has_alt_m12l = facts[i++]; f.cells_differ = facts[i++];
    f.grid_points_fused_ok = facts[i++]; f.match_small_ok_K = facts[i++]; f.match_small_ok_M = facts[i++];
    f.pose_inline_sync_ok = facts[i++]; f.pose_batch_kernel_selected = facts[i++]; f.pose_start_flag_ok = facts[i++];
    f.pose2p_waves_per_pair = facts[i++];
    stvo::DebugSwitches& d = f.sw;
    i = 0;
    d.pose_kernel = sw[i++]; d.seq_inline = sw[i++]; d.line_fused = sw[i++]; d.match_small = sw[i++]; d.match_lazy = sw[i++];
    d.grid_tail = sw[i++]; d.cells_ahead = sw[i++]; d.lines_ahead = sw[i++]; d.grid_cells = sw[i++];
    stvo::StepHistory h;
    h.fork_rec_frame = hist[0]; h.pose_flag_frame = hist[1]; h.sl_forked_frame = hist[2];
    int asked = 0, asked_bytes = 0;
    const stvo::StepPlan p = stvo::plan_step(f, h, [&](int bytes) {
        ++asked;
        asked_bytes = bytes;
        return lds_fits != 0;
    });
    if (do_commit) {
        stvo::commit(h, p, f.frame_idx);
        hist[0] = h.fork_rec_frame; hist[1] = h.pose_flag_frame; hist[2] = h.sl_forked_frame;
    }
    i = 0;
    out[i++] = p.light; out[i++] = p.par; out[i++] = p.mid_fork; out[i++] = p.fork_at_start; out[i++] = p.line_forked; out[i++] = p.zero_nl;
    out[i++] = p.point_stage; out[i++] = p.line_stage; out[i++] = p.clear_nl;
    out[i++] = p.lean_cells; out[i++] = p.has_tail; out[i++] = p.fused_cells; out[i++] = p.cells_ahead; out[i++] = p.lines_ahead; out[i++] = p.gate;
    out[i++] = p.Mk; out[i++] = (int)p.line_lds; out[i++] = p.line_fused;
    out[i++] = (int)p.match_points.route; out[i++] = p.match_points.small_cap; out[i++] = p.match_points.nseg_cap;
    out[i++] = (int)p.match_lines.route; out[i++] = p.match_lines.small_cap; out[i++] = p.match_lines.nseg_cap;
    out[i++] = p.track; out[i++] = p.match_lines_run; out[i++] = p.clear_m12l; out[i++] = p.use_alt_m12l;
    out[i++] = p.inline_sync; out[i++] = p.fetch_by_pose; out[i++] = p.inl_zero_copy; out[i++] = p.lazy_eig; out[i++] = p.pose_flagged;
    out[i++] = p.join_signal; out[i++] = p.fetch_copy; out[i++] = p.inl_copy;
    for (int k = 0; k < 8; ++k) out[i++] = p.schedule[k];
    out[i++] = asked; out[i++] = asked_bytes;
}

int sph_lsf_max_lines() { return stvo::LSF_MAX_LINES; }

}  // extern "C"
