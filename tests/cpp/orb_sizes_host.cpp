// The product's csrc/orb_sizes.h on the host, for tests/test_orb_sizes_host.py — TEST INFRASTRUCTURE ONLY.
#include <cstdint>

#include "../../stvo-pl_amd/csrc/orb_sizes.h"

extern "C" {

int osh_row_bytes() { return (int)sizeof(stvo::OrbLevelSize); }

void osh_budgets(int nfeatures, int nlevels, double scale_factor, int32_t* nf) {
    int v[64];
    stvo::orb_level_budgets(nfeatures, nlevels, scale_factor, v);
    for (int l = 0; l < nlevels; ++l) nf[l] = v[l];
}

// the table rows of one image size, field by field
void osh_level_sizes(int cols, int rows, int nfeatures, int nlevels, double scale_factor, int edge_th, int32_t* lcols, int32_t* lrows,
                     double* inv_sx, double* inv_sy, int32_t* active) {
    int nf[64];
    stvo::OrbLevelSize t[64];
    stvo::orb_level_budgets(nfeatures, nlevels, scale_factor, nf);
    stvo::orb_level_sizes(cols, rows, nlevels, scale_factor, edge_th, nf, t);
    for (int l = 0; l < nlevels; ++l) {
        lcols[l] = t[l].cols;
        lrows[l] = t[l].rows;
        inv_sx[l] = t[l].inv_sx;
        inv_sy[l] = t[l].inv_sy;
        active[l] = t[l].active;
    }
}

int osh_sizes_ok(const int32_t* sizes, int n, int B, int slot_cols, int slot_rows, int edge_th) {
    return stvo::orb_image_sizes_ok(sizes, n, B, slot_cols, slot_rows, edge_th) ? 1 : 0;
}

}  // extern "C"
