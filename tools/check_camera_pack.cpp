// check_camera_pack.cpp -- a stand-alone host program over the one host packer of cameras into kernel arguments
// (csrc/nbp_camera.h::cams_from_host): for every slot count the kernels use and every n = 1 .. n_slots, the first n slots hold R and
// T of their cameras split at word 9, the slots at or beyond n are all zero, and nothing beyond the 12 n input floats is read (the
// input is an exact-size heap block: an over-read is a sanitizer report).  It needs no GPU and is meant to run under the HOST
// sanitizers, from the repository root:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//         -I include -I nextbestpath_amd/csrc -x hip tools/check_camera_pack.cpp -o check_camera_pack
//   ./check_camera_pack   # "camera packing as expected", exit status 0, and no sanitizer report
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <hip/hip_runtime.h>
#include "nbp_camera.h"

static int fails = 0;
#define EXPECT(cond)                                                              \
    do {                                                                          \
        if (!(cond)) { printf("FAIL line %d: %s\n", __LINE__, #cond); ++fails; }  \
    } while (0)

static void check(int n_slots) {
    for (int n = 1; n <= n_slots; ++n) {
        float* in = (float*)malloc(sizeof(float) * 12 * (size_t)n);              // exactly 12 n floats
        for (int i = 0; i < 12 * n; ++i) in[i] = 1000.f + (float)i;              // every word its own value, none zero
        Cam* slots = (Cam*)malloc(sizeof(Cam) * (size_t)n_slots);
        memset(slots, 0xAB, sizeof(Cam) * (size_t)n_slots);                      // stale content must not survive
        cams_from_host(in, n, slots, n_slots);
        for (int f = 0; f < n_slots; ++f) {
            for (int k = 0; k < 9; ++k) EXPECT(slots[f].R[k] == (f < n ? in[12 * f + k] : 0.f));
            for (int k = 0; k < 3; ++k) EXPECT(slots[f].T[k] == (f < n ? in[12 * f + 9 + k] : 0.f));
        }
        free(slots);
        free(in);
    }
}

int main() {
    static_assert(sizeof(Cam) == 48, "a camera is twelve floats");
    static_assert(sizeof(CamSet) == MAX_CAMS * sizeof(Cam), "a camera set is its slots, nothing between them");
    check(MAX_CAMS);    // the simulator's and the splat's CamSet
    check(4);           // the step's batch items and a TSDF item's frames
    check(1);
    if (fails) { printf("%d check(s) failed\n", fails); return 1; }
    printf("camera packing as expected\n");
    return 0;
}
