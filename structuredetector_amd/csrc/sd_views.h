// What the test-time-augmentation files share (sd_tta.hip: the flip views, sd_d4.hip: the transposed views): the view table, its host
// check, and the tile of the merge + NMS kernels.
#pragma once
#include "sd_common.h"

namespace sd {

struct ViewFlips {
    unsigned char f[4];          // bit 0 = horizontal, bit 1 = vertical (the encoding of sd_preprocess_images' `flips`)
};

// One 256-thread block per 64x16 output tile of one merged map (the tile of sd_nms5), staged with its 2-pixel halo.
// LDS column of map column x: x - tx0 + OFF (OFF = 4) in the 16-byte and the 4-byte variants.
constexpr int TW = 64, TH = 16, HALO = 2, OFF = 4;
constexpr int LH = TH + 2 * HALO;        // 20 staged rows
constexpr int LWV = TW + 2 * OFF;        // 72 staged columns (VEC); the scalar variant fills columns OFF-HALO .. OFF+TW+HALO-1
constexpr int LWS = TW + 2 * HALO;       // 68 cells per row loaded by the scalar variant

static inline int check_views(const char* fn, int V, const unsigned char* view_flips, ViewFlips* vf, bool single_view = false) {
    SD_REQUIRE(V == 2 || V == 4 || (single_view && V == 1), SD_ERR_INVALID, "%s: V=%d views (%s are supported)", fn, V,
               single_view ? "1, 2 or 4" : "2 or 4");
    SD_REQUIRE(view_flips != nullptr, SD_ERR_INVALID, "%s: null view_flips", fn);
    *vf = ViewFlips{{0, 0, 0, 0}};
    for (int v = 0; v < V; ++v) {
        SD_REQUIRE(view_flips[v] < 4, SD_ERR_INVALID, "%s: view_flips[%d]=%d (bit 0 = horizontal, bit 1 = vertical)", fn, v, (int)view_flips[v]);
        vf->f[v] = view_flips[v];
    }
    SD_REQUIRE(view_flips[0] == 0, SD_ERR_INVALID, "%s: view 0 must be the unflipped image (view_flips[0]=%d)", fn, (int)view_flips[0]);
    return 0;
}

}  // namespace sd
