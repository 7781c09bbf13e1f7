// nbp_nn_grid.h -- the host side of the shell-walk grids: the grid over a caller's box, the argument checks and the carving of a
// plan and of its build scratch that the nearest-neighbour plan (nbp_recon.hip) and the triangle plan (nbp_surface.hip) share, so
// that both walk the SAME cells and the early exit's proof (nbp_shell_walk.h's header, beside the walk) covers both.  Included
// inside each translation unit; not part of the C ABI.
#pragma once
#include "nbp_grid.h"

#include <math.h>
#include <stddef.h>

namespace {

constexpr int NN_MAX_AXIS = 2048;                // cells per axis for which the early exit is proven (nbp_shell_walk.h's header)

struct Box { float hi[3]; };
struct BoxGrid { Grid g; Box bx; size_t ncell; };

bool nn_args_ok(const float* lo, const float* hi, float w) { return lo && hi && w > 0 && isfinite(w); }
// cap > 0 and at most 2^24 cells: the shell index and the cell coordinates stay inside int and exact in float
bool nn_cap_ok(float cap, float w) { return cap > 0 && isfinite(cap) && (double)cap / (double)w <= 16777216.0; }
// a count of points, triangles or vertices that indexes as an int
bool nn_count_ok(long long n) { return n >= 0 && n <= 0x7fffffffll; }

// The checked grid of an entry point over the caller's box [lo, hi]: cells 1.001 w wide (inv), one cell on an axis with hi == lo.
// NBP_E_ARG unless nn_args_ok, then NBP_E_ARG or NBP_E_SHAPE by the extents.  The entry's other NBP_E_ARG checks stand before it,
// its NBP_E_WS checks after it.
int nn_grid(const float* lo, const float* hi, float w, BoxGrid* b) {
    if (!nn_args_ok(lo, hi, w)) return NBP_E_ARG;
    size_t n = 1;
    for (int a = 0; a < 3; ++a) {
        b->g.lo[a] = lo[a];
        b->bx.hi[a] = hi[a];
        const double ext = (double)hi[a] - (double)lo[a];
        if (!(ext >= 0) || !(ext / (double)w < (double)NN_MAX_AXIS * 65536.0)) return ext >= 0 ? NBP_E_SHAPE : NBP_E_ARG;
        const long long na = (long long)(ext / (double)w) + 1;
        if (na > NN_MAX_AXIS) return NBP_E_SHAPE;
        b->g.n[a] = (int)na;
        n *= (size_t)na;
    }
    b->g.inv = (float)(1.0 / ((double)w * 1.001));
    if (n > (size_t)1 << 28) return NBP_E_SHAPE;
    b->ncell = n;
    return 0;
}

// A plan: `start` [ncell + 1], then `n_payload` float4 of payload (sorted points, or triangles' vertices).
struct NNPlan { int* start; float4* payload; };
NNPlan nn_plan_layout(Carver& c, size_t ncell, size_t n_payload) { return {c.take<int>(ncell + 1), c.take<float4>(n_payload)}; }
NNPlan nn_plan_of(const void* plan, size_t ncell) { return carve(plan, nn_plan_layout, ncell, (size_t)0); }       // (a reader needs no payload size)

// A build's scratch: the per-cell counts and the scan's tile sums; a build's own tail follows on the same carver.
struct NNScratch { int* count; int* tsum; };
NNScratch nn_scratch_layout(Carver& c, size_t ncell) { return {c.take<int>(ncell), take_scan_tsum(c, ncell)}; }
size_t nn_scratch_bytes(size_t ncell) { return carved_bytes(0, nn_scratch_layout, ncell); }

}  // namespace
