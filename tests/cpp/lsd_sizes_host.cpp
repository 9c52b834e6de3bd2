// The product's csrc/lsd_sizes.h on the host, for tests/test_lsd_sizes_host.py — TEST INFRASTRUCTURE ONLY.
#include <cstdint>

#include "../../stvo-pl_amd/csrc/lsd_sizes.h"

extern "C" {

int lsh_row_bytes() { return (int)sizeof(stvo::LsdSizeRow); }

// the table row of one image size, field by field, and the two rows that drive the blur and the resize
void lsh_row(int cols, int rows, double scale, double ang_th, double min_length, int32_t* out /* cols, rows, w, h, min_reg_size */,
             double* min_length_out, int32_t* srows /* [2][3] = cols, rows, active */, double* sinv /* [2][2] = inv_sx, inv_sy */) {
    const stvo::LsdSizeRow e = stvo::lsd_size_row(cols, rows, scale, ang_th, min_length);
    out[0] = e.cols; out[1] = e.rows; out[2] = e.w; out[3] = e.h; out[4] = e.min_reg_size;
    *min_length_out = e.min_length;
    stvo::OrbLevelSize s[2];
    stvo::lsd_scale_rows(e, scale, s);
    for (int i = 0; i < 2; ++i) {
        srows[3 * i] = s[i].cols; srows[3 * i + 1] = s[i].rows; srows[3 * i + 2] = s[i].active;
        sinv[2 * i] = s[i].inv_sx; sinv[2 * i + 1] = s[i].inv_sy;
    }
}

double lsh_scaled_extent(int n, double scale) { return stvo::lsd_scaled_extent(n, scale); }
int lsh_min_reg_size(int w, int h, double ang_th) { return stvo::lsd_min_reg_size(w, h, ang_th); }
double lsh_inv_ratio(double scale) { return stvo::lsd_inv_ratio(scale); }
double lsh_entry_min_length(const double* ml, int i, double own) { return stvo::lsd_entry_min_length(ml, i, own); }

int lsh_sizes_ok(const int32_t* sizes, const double* ml, int n, int B, int slot_cols, int slot_rows, double scale) {
    return stvo::lsd_image_sizes_ok(sizes, ml, n, B, slot_cols, slot_rows, scale) ? 1 : 0;
}
int lsh_lbd_sizes_ok(const int32_t* sizes, int n, int B, int slot_cols, int slot_rows) {
    return stvo::lbd_image_sizes_ok(sizes, n, B, slot_cols, slot_rows) ? 1 : 0;
}

}  // extern "C"
