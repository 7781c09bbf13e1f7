// check_workspace_carve.cpp -- a stand-alone host program over the workspace carver (csrc/nbp_carve.h) and the workspace refusals
// of every entry point that carves one: a call with one byte less than its *_bytes function asks for, or with none, is refused
// with NBP_E_WS before a launch.  It needs no GPU and is meant to run under the HOST sanitizers, from the repository root:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//         -I include -I nextbestpath_amd/csrc -x hip tools/check_workspace_carve.cpp nextbestpath_amd/csrc/nbp_sim.hip \
//         nextbestpath_amd/csrc/nbp_planner.hip nextbestpath_amd/csrc/nbp_scene.hip nextbestpath_amd/csrc/nbp_recon.hip \
//         nextbestpath_amd/csrc/nbp_surface.hip nextbestpath_amd/csrc/nbp_maps.hip nextbestpath_amd/csrc/nbp_tuning.cpp -o check_carve
//   ./check_carve       # "carver and refusals as expected", exit status 0, and no sanitizer report
// The device code is not instrumented, and nothing here reaches it: host buffers stand in for device memory.
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include "nbp_hip.h"
#include "nbp_carve.h"

static int fails = 0;
#define EXPECT(call, want)                                                        \
    do {                                                                          \
        const long long got = (long long)(call);                                  \
        if (got != (long long)(want)) { printf("FAIL %s: %lld != %lld\n", #call, got, (long long)(want)); ++fails; } \
    } while (0)
// refused one byte short and with no bytes at all (NBYTES is the name the call uses for the size under test)
#define REFUSED(bytes_fn, call)                                                   \
    do {                                                                          \
        const size_t full = (bytes_fn);                                           \
        EXPECT(full > 0, 1);                                                      \
        size_t NBYTES = full - 1;                                                 \
        EXPECT(call, NBP_E_WS);                                                   \
        NBYTES = 0;                                                               \
        EXPECT(call, NBP_E_WS);                                                   \
    } while (0)

// a layout with odd counts and element sizes; returns each buffer's [begin, end)
struct Taken { char* p[4]; size_t n[4]; };
static Taken layout(Carver& c) {
    Taken t;
    t.n[0] = 13 * 4; t.p[0] = (char*)c.take<int>(13);
    t.n[1] = 1 * 8; t.p[1] = (char*)c.take<double>(1);
    t.n[2] = 256; t.p[2] = (char*)c.take<char>(256);
    t.n[3] = 257; t.p[3] = (char*)c.take<char>(257);
    return t;
}

static void check_carver() {
    Carver dry;
    layout(dry);
    EXPECT(dry.dry(), 1);
    EXPECT(dry.end(), 256 + 256 + 256 + 512);
    EXPECT(dry.bytes(), 256 + dry.end());
    EXPECT(dry.bytes(512), 256 + dry.end() + 512);
    const size_t nbytes = dry.bytes();
    char* block = (char*)aligned_alloc(256, nbytes + 256);
    const int skew[4] = {0, 1, 8, 255};
    for (int s = 0; s < 4; ++s) {
        char* ws = block + skew[s];                              // the caller's workspace: nbytes from here
        Carver live(ws);
        const Taken t = layout(live);
        EXPECT(live.dry(), 0);
        EXPECT(live.end(), dry.end());                           // dry and live runs give equal offsets
        EXPECT((uintptr_t)live.base - (uintptr_t)ws < 256, 1);
        size_t off = 0;
        for (int i = 0; i < 4; ++i) {
            EXPECT((uintptr_t)t.p[i] & 255, 0);
            EXPECT(t.p[i] - live.base, off);
            off += Carver::round256(t.n[i]);
            EXPECT(t.p[i] >= ws && t.p[i] + t.n[i] <= ws + nbytes, 1);     // the last buffer too ends inside bytes()
            for (size_t k = 0; k < t.n[i]; ++k) t.p[i][k] = (char)i;        // (the sanitizer watches the block's ends)
        }
    }
    free(block);
}

int main() {
    check_carver();

    // host buffers stand in for device memory: a refused call dereferences none of them
    void* dev = aligned_alloc(4096, 1 << 16);
    float* f = (float*)dev; int* ip = (int*)dev; long long* ll = (long long*)dev;
    float cams[12 * 4 * 2] = {0};
    const float lo[3] = {0.f, 0.f, 0.f}, hi[3] = {4.f, 3.f, 5.f};
    const float box6[6] = {0.f, 0.f, 0.f, 4.f, 3.f, 5.f};
    const int grid3[3] = {2, 2, 2};
    const float lo2[2] = {0.f, 0.f}, hi2[2] = {40.f, 30.f};

    // ---- un-projection: one entry per colour source, and the batch of two items
    REFUSED(nbp_unproject_workspace_bytes(1, 8, 12),
            nbp_unproject_append_f32(f, nullptr, cams, 1, 8, 12, 0.5f, 10.f, 0.5, 1u, ip, f, ll, 100, dev, NBYTES, nullptr));
    REFUSED(nbp_unproject_workspace_bytes(4, 7, 9),
            nbp_unproject_append_rgb_f32(f, nullptr, f, cams, 4, 7, 9, 0.5f, 10.f, 0.5, 1u, ip, f, f, ll, 100, dev, NBYTES, nullptr));
    REFUSED(nbp_unproject_workspace_bytes(4, 8, 12),
            nbp_unproject_append_shaded_f32(f, nullptr, dev, f, ip, f, cams, 4, 8, 12, 0.5f, 10.f, 0.5, 1u, 0.85f, ip, f, f, ll, 100, dev,
                                            NBYTES, nullptr));
    REFUSED(nbp_unproject_workspace_bytes(1, 8, 12),
            nbp_unproject_append_filed_f32(f, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, cams, 1, 8, 12, 0.5f, 10.f, 0.5, 1u,
                                           0.85f, ip, f, nullptr, ll, 100, dev, nullptr, nullptr, 64, dev, NBYTES, nullptr));
    {
        const float* depth[4] = {f, f, f, f};
        const unsigned seeds[2] = {1u, 2u};
        int* counts2[2] = {ip, ip};
        float* cloud[2] = {f, f};
        long long* cloud_count[2] = {ll, ll};
        const long long capacity[2] = {100, 100};
        void* ws[2] = {dev, dev};
        REFUSED(nbp_unproject_workspace_bytes(2, 8, 12),
                nbp_unproject_append_shaded_batch_f32(2, depth, nullptr, nullptr, nullptr, nullptr, cams, 2, 8, 12, 0.5f, 10.f, 0.5, seeds,
                                                      0.85f, counts2, cloud, nullptr, cloud_count, capacity, ws, NBYTES, nullptr));
    }
    // ---- rasteriser: depth only, coloured, (depth, face) images, and the batch (an item's own size is the one under test)
    REFUSED(nbp_raster_workspace_bytes(13, 2, 24, 40, 0),
            nbp_raster_zbuf_f32(f, 8, ip, 13, cams, 2, 24, 40, 0.5f, 0.01f, 0, f, nullptr, dev, NBYTES, nullptr));
    REFUSED(nbp_raster_rgb_workspace_bytes(13, 2, 24, 40),
            nbp_raster_rgbz_f32(f, 8, ip, 13, f, cams, 2, 24, 40, 0.5f, 0.01f, 0.85f, 1.5f, f, f, dev, NBYTES, nullptr));
    REFUSED(nbp_raster_workspace_bytes(12, 2, 24, 40, 0),
            nbp_raster_zface_f32(f, 8, ip, 12, cams, 2, 24, 40, 0.5f, 0.01f, f, dev, dev, NBYTES, nullptr));
    {
        const float* verts[2] = {f, f};
        const int n_verts[2] = {8, 8}, n_faces[2] = {12, 13};
        const int* faces[2] = {ip, ip};
        float* zbuf[2] = {f, f};
        void* zface[2] = {dev, dev};
        void* ws[2] = {dev, dev};
        size_t ws_bytes[2] = {nbp_raster_workspace_bytes(12, 2, 24, 40, 0), 0};
        REFUSED(nbp_raster_workspace_bytes(13, 2, 24, 40, 0),
                (ws_bytes[1] = NBYTES, nbp_raster_zface_batch_f32(2, verts, n_verts, faces, n_faces, cams, 2, 24, 40, 0.5f, 0.01f, zbuf, zface,
                                                                  ws, ws_bytes, nullptr)));
    }
    // ---- coverage: the one-shot count, and the plan build's plan and scratch
    REFUSED(nbp_coverage_workspace_bytes(lo, hi, 1.f, 100),
            nbp_coverage_count_f32(f, 50, f, 200, nullptr, 100, 1u, 1.f, lo, hi, ip, ip, dev, NBYTES, nullptr));
    const size_t cov_plan = nbp_coverage_plan_bytes(lo, hi, 1.f, 50), cov_ws = nbp_coverage_plan_workspace_bytes(lo, hi, 1.f, 50);
    REFUSED(cov_plan, nbp_coverage_plan_build_f32(f, 50, 1.f, lo, hi, dev, NBYTES, dev, cov_ws, nullptr));
    REFUSED(cov_ws, nbp_coverage_plan_build_f32(f, 50, 1.f, lo, hi, dev, cov_plan, dev, NBYTES, nullptr));
    // ---- scene store
    REFUSED(nbp_scene_fill_workspace_bytes(box6, grid3, 16, 100, 0.5),
            nbp_scene_fill_cells_f32(f, 100, nullptr, box6, grid3, 16, 0.5, 0, 1u, f, ip, dev, NBYTES, nullptr));
    REFUSED(nbp_scene_coverage_workspace_bytes(box6, grid3, 16, 0.5),
            nbp_scene_coverage_f32(f, ip, 16, f, ip, 16, box6, grid3, 0.5, ip, dev, NBYTES, nullptr));
    // ---- shell-walk grids: the point plan, the one-shot query, the triangle plan's two passes
    const size_t nn_plan = nbp_nn_plan_bytes(lo, hi, 1.f, 50), nn_ws = nbp_nn_plan_workspace_bytes(lo, hi, 1.f, 50);
    REFUSED(nn_plan, nbp_nn_plan_build_f32(f, 50, nullptr, lo, hi, 1.f, dev, NBYTES, dev, nn_ws, nullptr));
    REFUSED(nn_ws, nbp_nn_plan_build_f32(f, 50, nullptr, lo, hi, 1.f, dev, nn_plan, dev, NBYTES, nullptr));
    REFUSED(nbp_nn_dist2_workspace_bytes(lo, hi, 1.f, 50),
            nbp_nn_dist2_f32(f, 64, nullptr, f, 50, nullptr, lo, hi, 2.f, 1.f, f, dev, NBYTES, nullptr));
    const size_t mesh_plan = nbp_mesh_plan_bytes(lo, hi, 1.f, 12), mesh_ws = nbp_mesh_plan_workspace_bytes(lo, hi, 1.f);
    REFUSED(mesh_plan, nbp_mesh_plan_count_f32(f, 8, ip, 12, lo, hi, 1.f, dev, NBYTES, ll, dev, mesh_ws, nullptr));
    REFUSED(mesh_ws, nbp_mesh_plan_count_f32(f, 8, ip, 12, lo, hi, 1.f, dev, mesh_plan, ll, dev, NBYTES, nullptr));
    REFUSED(mesh_ws, nbp_mesh_plan_fill_i32(f, 8, ip, 12, lo, hi, 1.f, dev, ip, 100, dev, NBYTES, nullptr));
    // ---- cloud bins: the store itself
    REFUSED(nbp_cloud_bins_bytes(lo2, hi2, 1000), nbp_cloud_bins_init(dev, NBYTES, lo2, hi2, 1000, nullptr));

    free(dev);
    printf(fails ? "%d FAILED\n" : "carver and refusals as expected (%d failures)\n", fails);
    return fails != 0;
}
