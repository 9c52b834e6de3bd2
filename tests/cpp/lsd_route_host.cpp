// The product's csrc/lsd_route.h on the host, for tests/test_lsd_route_host.py — TEST INFRASTRUCTURE ONLY.
#include "../../stvo-pl_amd/csrc/lsd_route.h"

extern "C" {

// the decision for one combination of the facts: search | refine << 8 | prof << 9
int lrh_route(int refine, int arena, int table, int table_route, int lsd_grow, int probes) {
    const stvo::LsdRoute r = stvo::lsd_search_route(stvo::LsdRouteFacts{refine, arena != 0, table != 0, table_route, lsd_grow, probes != 0});
    return r.search | ((r.refine ? 1 : 0) << 8) | ((r.prof ? 1 : 0) << 9);
}

int lrh_table_route_ok(int route) { return stvo::lsd_table_route_ok(route) ? 1 : 0; }

// the values, in the order ONE_WAVE, ONE_WAVE_PLAIN, MANY_WAVES, TABLE_ONE_WAVE, TABLE_BY_BATCH
void lrh_values(int* out) {
    out[0] = stvo::LSD_SEARCH_ONE_WAVE; out[1] = stvo::LSD_SEARCH_ONE_WAVE_PLAIN; out[2] = stvo::LSD_SEARCH_MANY_WAVES;
    out[3] = stvo::LSD_TABLE_ONE_WAVE; out[4] = stvo::LSD_TABLE_BY_BATCH;
}

}  // extern "C"
