// The product's csrc/fld_sizes.h on the host, as a program of its own for tests/test_fld_sizes_host.py (plain, and under
// -fsanitize=address,undefined) — TEST INFRASTRUCTURE ONLY.  Reads queries from standard input, one per line, answers one line each:
//   row  cols rows L                              -> row cols rows npx nw nunits L bytes
//   grid c0 c1 r0 r1 L                            -> one `row` line per size c0 <= cols <= c1, r0 <= rows <= r1 (cols outermost)
//   ok   slot_cols slot_rows L_det B n own (cols rows [L])*n   (own = 1: a threshold per entry follows each size; 0: none, NULL)
//                                                 -> ok verdict entry need have ok_bool   (verdict 0 taken, 1 invalid, 2 capacity)
// The lists are held in heap blocks of exactly n entries, so that a read past either end is the sanitizer's to report.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>

#include "../../stvo-pl_amd/csrc/fld_sizes.h"

static void print_row(int cols, int rows, int L) {
    const stvo::FldSizeRow e = stvo::fld_size_row(cols, rows, L);
    std::printf("row %d %d %d %d %d %d %d\n", e.cols, e.rows, e.npx, e.nw, e.nunits, e.L, (int)sizeof(e));
}

int main() {
    char cmd[16];
    while (std::scanf("%15s", cmd) == 1) {
        if (!std::strcmp(cmd, "row")) {
            int c, r, L;
            if (std::scanf("%d %d %d", &c, &r, &L) != 3) return 2;
            print_row(c, r, L);
        } else if (!std::strcmp(cmd, "grid")) {
            int c0, c1, r0, r1, L;
            if (std::scanf("%d %d %d %d %d", &c0, &c1, &r0, &r1, &L) != 5) return 2;
            for (int c = c0; c <= c1; ++c)
                for (int r = r0; r <= r1; ++r) print_row(c, r, L);
        } else if (!std::strcmp(cmd, "ok")) {
            int sc, sr, Ld, B, n, own;
            if (std::scanf("%d %d %d %d %d %d", &sc, &sr, &Ld, &B, &n, &own) != 6) return 2;
            const int m = n > 0 ? n : 0;
            std::unique_ptr<int32_t[]> sizes(new int32_t[2 * (size_t)m]), L(new int32_t[(size_t)m]);
            for (int i = 0; i < m; ++i) {
                if (std::scanf("%d %d", &sizes[2 * i], &sizes[2 * i + 1]) != 2) return 2;
                if (own && std::scanf("%d", &L[i]) != 1) return 2;
            }
            int entry = -1, need = -1, have = -1;
            const int v = (int)stvo::fld_image_sizes_verdict(sizes.get(), own ? L.get() : nullptr, n, B, sc, sr, Ld, &entry, &need, &have);
            const bool ok = stvo::fld_image_sizes_ok(sizes.get(), own ? L.get() : nullptr, n, B, sc, sr, Ld);
            std::printf("ok %d %d %d %d %d\n", v, entry, need, have, ok ? 1 : 0);
        } else {
            return 2;
        }
    }
    // a null list is refused before it is read
    if (stvo::fld_image_sizes_ok(nullptr, nullptr, 1, 1, 160, 120, 6)) return 3;
    std::printf("end\n");
    return 0;
}
