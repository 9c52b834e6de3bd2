// lsd_route.h — which search kernel the LSD detector's next detection launches, host-pure (no HIP): ONE function from the facts to the
// kernel, called by lsd_enqueue (which launches what it says) and by stvo_lsd_search_route (which reports it).  The values are those of
// include/stvo_hip.h; they are restated here so that the header compiles alone on the host (tests/cpp/lsd_route_host.cpp runs it over
// every combination of its facts, tests/test_lsd_route_host.py), and lsd_kernels.hip asserts that the two agree.
//   lsd_refine = 1                 the plain one-wave kernel with refinement (lsd_grow_refine_kernel<true>) whatever else holds: regions
//                                  give pixels back, which the other forms do not survive
//   the detector holds the arena   (created for <= 128 images of <= LSD_XCD_MAX_PX scaled pixels without refinement — lsd_xcd_route — and
//                                  not under STVO_LSD_WAVES=0): the many-wave search, lsd_grow_xcd_kernel — with no table always; under
//                                  a size table only where the caller chose STVO_LSD_TABLE_BY_BATCH (stvo_lsd_set_table_route), the
//                                  default STVO_LSD_TABLE_ONE_WAVE being the contract tables had from the start
//   STVO_LSD_GROW=0                the plain one-wave kernel without refinement (lsd_grow_refine_kernel<false>), the cross-check
//   else                           lsd_grow_kernel, one wave per image
// The probes (stvo_lsd_debug) never change the search; they choose the PROF instance of its kernel, which exists only with no table.
#pragma once

namespace stvo {

constexpr int LSD_SEARCH_ONE_WAVE = 0;        // STVO_LSD_SEARCH_ONE_WAVE        lsd_grow_kernel
constexpr int LSD_SEARCH_ONE_WAVE_PLAIN = 1;  // STVO_LSD_SEARCH_ONE_WAVE_PLAIN  lsd_grow_refine_kernel, with or without refinement
constexpr int LSD_SEARCH_MANY_WAVES = 2;      // STVO_LSD_SEARCH_MANY_WAVES      lsd_grow_xcd_kernel
constexpr int LSD_TABLE_ONE_WAVE = 0;         // STVO_LSD_TABLE_ONE_WAVE
constexpr int LSD_TABLE_BY_BATCH = 1;         // STVO_LSD_TABLE_BY_BATCH

struct LsdRouteFacts {
    int refine;        // stvo_lsd_params::refine
    bool arena;        // the detector holds the small-batch arena of lsd_grow_xcd_kernel
    bool table;        // a size table is in force (stvo_lsd_set_image_sizes)
    int table_route;   // LSD_TABLE_* (stvo_lsd_set_table_route)
    int lsd_grow;      // STVO_LSD_GROW (0: the plain form)
    bool probes;       // stvo_lsd_debug has the probes on
};

struct LsdRoute {
    int search;   // LSD_SEARCH_*
    bool refine;  // the plain kernel's REFINE instance
    bool prof;    // the PROF instance of the search kernel
};

inline bool lsd_table_route_ok(int route) { return route == LSD_TABLE_ONE_WAVE || route == LSD_TABLE_BY_BATCH; }

inline LsdRoute lsd_search_route(const LsdRouteFacts& f) {
    LsdRoute r;
    r.refine = f.refine == 1;
    r.prof = f.probes && !f.table && !r.refine;  // (no PROF instance under a table, none of the refining kernel)
    if (r.refine) r.search = LSD_SEARCH_ONE_WAVE_PLAIN;
    else if (f.arena && (!f.table || f.table_route == LSD_TABLE_BY_BATCH)) r.search = LSD_SEARCH_MANY_WAVES;
    else if (f.lsd_grow == 0) r.search = LSD_SEARCH_ONE_WAVE_PLAIN;
    else r.search = LSD_SEARCH_ONE_WAVE;
    return r;
}

}  // namespace stvo
