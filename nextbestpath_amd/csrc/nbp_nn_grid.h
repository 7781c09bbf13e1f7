// nbp_nn_grid.h -- the host side of the shell-walk grids: the grid over a caller's box and the argument checks that the
// nearest-neighbour plan (nbp_recon.hip) and the triangle plan (nbp_surface.hip) share, so that both walk the SAME cells and the
// early exit's proof (nbp_recon.hip's header) covers both.  Included inside each translation unit; not part of the C ABI.
#pragma once
#include "nbp_grid.h"

#include <math.h>
#include <stddef.h>

namespace {

constexpr int NN_MAX_AXIS = 2048;                // cells per axis for which the early exit is proven (nbp_recon.hip's header)

struct Box { float hi[3]; };

static size_t al256(size_t b) { return (b + 255) / 256 * 256; }

// The grid over the caller's box [lo, hi]: cells 1.001 w wide (inv), one cell on an axis with hi == lo.
int nn_grid(const float* lo, const float* hi, float w, Grid* g, Box* bx, size_t* ncell) {
    size_t n = 1;
    for (int a = 0; a < 3; ++a) {
        g->lo[a] = lo[a];
        bx->hi[a] = hi[a];
        const double ext = (double)hi[a] - (double)lo[a];
        if (!(ext >= 0) || !(ext / (double)w < (double)NN_MAX_AXIS * 65536.0)) return ext >= 0 ? NBP_E_SHAPE : NBP_E_ARG;
        const long long na = (long long)(ext / (double)w) + 1;
        if (na > NN_MAX_AXIS) return NBP_E_SHAPE;
        g->n[a] = (int)na;
        n *= (size_t)na;
    }
    g->inv = (float)(1.0 / ((double)w * 1.001));
    if (n > (size_t)1 << 28) return NBP_E_SHAPE;
    *ncell = n;
    return 0;
}

bool nn_args_ok(const float* lo, const float* hi, float w) { return lo && hi && w > 0 && isfinite(w); }
// cap > 0 and at most 2^24 cells: the shell index and the cell coordinates stay inside int and exact in float
bool nn_cap_ok(float cap, float w) { return cap > 0 && isfinite(cap) && (double)cap / (double)w <= 16777216.0; }

}  // namespace
