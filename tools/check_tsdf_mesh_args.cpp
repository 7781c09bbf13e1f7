// check_tsdf_mesh_args.cpp -- a stand-alone host program over the argument checks of nbp_tsdf_mesh_f32 (csrc/nbp_tsdf_mesh.hip): every
// call here is refused before a launch, so it needs no GPU and is meant to run under the HOST sanitizers, from the repository root:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -fsanitize=address,undefined \
//         -I include -I nextbestpath_amd/csrc -x hip tools/check_tsdf_mesh_args.cpp nextbestpath_amd/csrc/nbp_tsdf_mesh.hip -o check_args
//   ./check_args        # "all refusals as expected", exit status 0, and no sanitizer report
// The device code is not instrumented, and nothing here reaches it.
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include "nbp_hip.h"

static int fails = 0;
#define EXPECT(call, want)                                                        \
    do {                                                                          \
        const long long got = (long long)(call);                                  \
        if (got != (long long)(want)) { printf("FAIL %s: %lld != %lld\n", #call, got, (long long)(want)); ++fails; } \
    } while (0)

static void* buf(size_t n) { return aligned_alloc(256, (n + 255) / 256 * 256); }

int main() {
    const int nx = 3, ny = 5, nz = 7;
    const long long nv = (long long)nx * ny * nz;
    const size_t nws = nbp_tsdf_mesh_workspace_bytes(nv);
    EXPECT(nws >= 256 + 16 + 4 * (size_t)nv, 1);
    EXPECT(nbp_tsdf_mesh_workspace_bytes(0), 0);
    EXPECT(nbp_tsdf_mesh_workspace_bytes(-5), 0);
    EXPECT(nbp_tsdf_mesh_workspace_bytes((1ll << 28) + 1), 0);
    EXPECT(nbp_tsdf_mesh_workspace_bytes(1ll << 28) > (size_t)(1ll << 30), 1);
    // host buffers stand in for device memory: a refused call dereferences none of them (lo is host memory by contract)
    int* vol = (int*)buf((size_t)nv * 8 + 256);
    float* verts = (float*)buf(64 * 12);
    int* faces = (int*)buf(64 * 12);
    float* area2 = (float*)buf(64 * 4);
    long long* totals = (long long*)buf(256);
    char* ws = (char*)buf(nws + 256);
    float lo[3] = {-0.5f, -0.5f, 2.0f}, bad_lo[3] = {0.f, __builtin_nanf(""), 0.f};
#define CALL(V, LO, VOX, NX, NY, NZ, MW, VE, VC, FA, AR, FC, TO, WS, NWS) \
    nbp_tsdf_mesh_f32(V, LO, VOX, NX, NY, NZ, MW, VE, VC, FA, AR, FC, TO, WS, NWS, nullptr)
    EXPECT(CALL(nullptr, lo, 0.3f, nx, ny, nz, 1, verts, 64, faces, area2, 64, totals, ws, nws), NBP_E_ARG);
    EXPECT(CALL(vol, nullptr, 0.3f, nx, ny, nz, 1, verts, 64, faces, area2, 64, totals, ws, nws), NBP_E_ARG);
    EXPECT(CALL(vol, bad_lo, 0.3f, nx, ny, nz, 1, verts, 64, faces, area2, 64, totals, ws, nws), NBP_E_ARG);
    EXPECT(CALL(vol, lo, 0.0f, nx, ny, nz, 1, verts, 64, faces, area2, 64, totals, ws, nws), NBP_E_ARG);
    EXPECT(CALL(vol, lo, 0.3f, nx, 0, nz, 1, verts, 64, faces, area2, 64, totals, ws, nws), NBP_E_ARG);
    EXPECT(CALL(vol, lo, 0.3f, nx, ny, nz, 0, verts, 64, faces, area2, 64, totals, ws, nws), NBP_E_ARG);
    EXPECT(CALL(vol, lo, 0.3f, nx, ny, nz, 1, verts, -1, faces, area2, 64, totals, ws, nws), NBP_E_ARG);
    EXPECT(CALL(vol, lo, 0.3f, nx, ny, nz, 1, verts, 64, faces, area2, -1, totals, ws, nws), NBP_E_ARG);
    EXPECT(CALL(vol, lo, 0.3f, nx, ny, nz, 1, nullptr, 64, faces, area2, 64, totals, ws, nws), NBP_E_ARG);
    EXPECT(CALL(vol, lo, 0.3f, nx, ny, nz, 1, verts, 64, nullptr, area2, 64, totals, ws, nws), NBP_E_ARG);
    EXPECT(CALL(vol, lo, 0.3f, nx, ny, nz, 1, verts, 64, faces, area2, 64, nullptr, ws, nws), NBP_E_ARG);
    EXPECT(CALL(vol, lo, 0.3f, nx, ny, nz, 1, verts, 64, faces, area2, 64, totals, nullptr, nws), NBP_E_ARG);
    EXPECT(CALL(vol, lo, 0.3f, nx, ny, nz, 1, verts, 64, faces, area2, 64, (long long*)((char*)totals + 4), ws, nws), NBP_E_SHAPE);
    EXPECT(CALL((int*)((char*)vol + 4), lo, 0.3f, nx, ny, nz, 1, verts, 64, faces, area2, 64, totals, ws, nws), NBP_E_SHAPE);
    EXPECT(CALL(vol, lo, 0.3f, 1 << 10, 1 << 10, (1 << 8) + 1, 1, verts, 64, faces, area2, 64, totals, ws, nws), NBP_E_SHAPE);
    EXPECT(CALL(vol, lo, 0.3f, 1 << 20, 1 << 20, 1 << 20, 1, verts, 64, faces, area2, 64, totals, ws, nws), NBP_E_SHAPE);
    EXPECT(CALL(vol, lo, 0.3f, nx, ny, nz, 1, verts, 64, faces, area2, 64, totals, ws, nws - 1), NBP_E_WS);
    EXPECT(CALL(vol, lo, 0.3f, nx, ny, nz, 1, verts, 64, faces, area2, 64, totals, ws, 0), NBP_E_WS);
    // overlaps: outputs, totals and workspace inside the volume; outputs on each other; an output inside the workspace in use
    EXPECT(CALL(vol, lo, 0.3f, nx, ny, nz, 1, (float*)vol, 64, faces, area2, 64, totals, ws, nws), NBP_E_ARG);
    EXPECT(CALL(vol, lo, 0.3f, nx, ny, nz, 1, verts, 64, vol + 2, area2, 64, totals, ws, nws), NBP_E_ARG);
    EXPECT(CALL(vol, lo, 0.3f, nx, ny, nz, 1, verts, 64, faces, (float*)(vol + 4), 64, totals, ws, nws), NBP_E_ARG);
    EXPECT(CALL(vol, lo, 0.3f, nx, ny, nz, 1, verts, 64, faces, area2, 64, (long long*)(vol + 2), ws, nws), NBP_E_ARG);
    EXPECT(CALL(vol, lo, 0.3f, nx, ny, nz, 1, verts, 64, faces, area2, 64, totals, vol, nws), NBP_E_ARG);
    EXPECT(CALL(vol, lo, 0.3f, nx, ny, nz, 1, verts, 64, (int*)verts, area2, 64, totals, ws, nws), NBP_E_ARG);
    EXPECT(CALL(vol, lo, 0.3f, nx, ny, nz, 1, verts, 64, faces, (float*)(faces + 2), 64, totals, ws, nws), NBP_E_ARG);
    EXPECT(CALL(vol, lo, 0.3f, nx, ny, nz, 1, (float*)(ws + 256), 64, faces, area2, 64, totals, ws, nws), NBP_E_ARG);
    // the last byte of the volume against the first of an output (one past the end is fine for the check itself: refused by ws)
    EXPECT(CALL(vol, lo, 0.3f, nx, ny, nz, 1, (float*)((char*)vol + nv * 8 - 4), 1, faces, area2, 64, totals, ws, nws), NBP_E_ARG);
    EXPECT(CALL(vol, lo, 0.3f, nx, ny, nz, 1, (float*)((char*)vol + nv * 8), 1, faces, area2, 64, totals, ws, nws - 1), NBP_E_WS);
    free(vol); free(verts); free(faces); free(area2); free(totals); free(ws);
    printf(fails ? "%d FAILED\n" : "all refusals as expected (%d failures)\n", fails);
    return fails != 0;
}
