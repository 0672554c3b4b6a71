// ma_table_entry_sweep.cpp - the descriptor checks, size checks and offset arithmetic of gadapt_ma_table_batch and
// gadapt_ma_table_batch_strided as a stand-alone host program for sanitizer builds.  mesh_csrc/ma_table_kernels.hip is compiled
// with -DGADAPT_MA_TABLE_NO_LAUNCH, which ends both entry points after their checks (no kernel is launched, no device is
// needed) and leaves the launch's thread count and dynamic LDS in g_sweep_threads / g_sweep_lds:
//   hipcc --offload-arch=gfx950 -std=c++17 -g -Iinclude -Ig_adaptivity_amd/mesh_csrc -ffp-contract=off -DGADAPT_MA_TABLE_NO_LAUNCH \
//       -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//       tools/ma_table_entry_sweep.cpp g_adaptivity_amd/mesh_csrc/ma_table_kernels.hip -o build/ma_table_entry_sweep
//   build/ma_table_entry_sweep
// Descriptors live in heap buffers of exactly the size they need, so a read past a batch's last word is a heap overflow.
// Prints the number of calls and exits 0, or says what was wrong and exits 1.
#include <stdint.h>
#include <stdio.h>
#include <limits.h>
#include <vector>
#include "gadapt_mesh.h"

extern int g_sweep_threads;
extern int64_t g_sweep_lds;

typedef int (*entry_t)(int, const int32_t*, const int32_t*, const float*, double, double, int, float*, float*, int32_t*, float*,
                       int32_t*, void*);

int main() {
    float dummy_f = 0.0f;
    int32_t dummy_i = 0;
    float* pf = &dummy_f;                                    // never dereferenced: nothing is launched
    int32_t* pi = &dummy_i;
    const entry_t entries[2] = {gadapt_ma_table_batch, gadapt_ma_table_batch_strided};
    const int sides[2] = {32, 81};
    if (gadapt_ma_table_max_side() != 1024) { printf("max side %d\n", gadapt_ma_table_max_side()); return 1; }
    const int ns[] = {INT_MIN, -1, 0, 2, 3, 8, 9, 31, 32, 33, 80, 81, 82, 46341, INT_MAX};
    const int ts[] = {INT_MIN, -1, 0, 1, 2, 3, 1023, 1024, 1025, 46341, INT_MAX};
    const int offs[] = {INT_MIN, -1, 0, 1, INT_MAX - 1024 * 1024 - 1, INT_MAX - 1024 * 1024, INT_MAX - 1024 * 1024 + 1, INT_MAX - 6561,
                        INT_MAX - 6560, INT_MAX - 4, INT_MAX - 3, INT_MAX};
    long calls = 0;
    for (int r = 0; r < 2; ++r)
    for (int B = 1; B <= 3; ++B)
    for (int N : ns) for (int T : ts) for (int noff : offs) for (int toff : offs) {
        std::vector<int32_t> desc((size_t)GADAPT_MA_DESC * B);
        for (int b = 0; b < B - 1; ++b) {                    // good meshes first: the one under test is the last of the batch
            desc[4 * b + GADAPT_MA_D_N] = 11, desc[4 * b + GADAPT_MA_D_NODE_OFF] = 121 * b;
            desc[4 * b + GADAPT_MA_D_TABLE_OFF] = 81 * b, desc[4 * b + GADAPT_MA_D_TABLE_T] = 9;
        }
        int32_t* d = desc.data() + 4 * (B - 1);
        d[GADAPT_MA_D_N] = N, d[GADAPT_MA_D_NODE_OFF] = noff, d[GADAPT_MA_D_TABLE_OFF] = toff, d[GADAPT_MA_D_TABLE_T] = T;
        const int rc = entries[r](B, desc.data(), pi, pf, 0.2, 1e-4, 100, pf, pf, pi, pf, pi, nullptr);
        ++calls;
        const bool bad = N < 3 || noff < 0 || toff < 0;
        const bool size = !bad && (N > sides[r] || T < 2 || T > 1024 ||
                                   (int64_t)noff + (int64_t)N * N > INT_MAX || (int64_t)toff + (int64_t)T * T > INT_MAX);
        const int want = bad ? GADAPT_MESH_E_BADARG : size ? GADAPT_MESH_E_SIZE : GADAPT_MESH_OK;
        if (rc != want) { printf("route %d B %d N %d T %d offsets %d / %d: %d, expected %d\n", r, B, N, T, noff, toff, rc, want); return 1; }
        if (rc == GADAPT_MESH_OK) {
            const int big = N > 11 || B == 1 ? N : 11, nodes = big * big, rounded = (nodes + 63) & ~63;
            const int threads = rounded < 1024 ? rounded : 1024;
            const int64_t lds = 256 + 8 * (int64_t)nodes;    // two fp32 images or one fp64 image
            if (g_sweep_threads != threads || g_sweep_lds != lds || lds > 65536) {
                printf("route %d N %d: %d threads, %lld bytes of LDS\n", r, N, g_sweep_threads, (long long)g_sweep_lds);
                return 1;
            }
        }
    }
    for (int r = 0; r < 2; ++r) {                            // the scalar arguments and the null pointers
        int32_t one[4] = {11, 0, 0, 9};
        if (entries[r](0, one, pi, pf, 0.2, 1e-4, 100, pf, pf, pi, pf, pi, nullptr) != GADAPT_MESH_E_BADARG) return 1;
        if (entries[r](1, nullptr, pi, pf, 0.2, 1e-4, 100, pf, pf, pi, pf, pi, nullptr) != GADAPT_MESH_E_BADARG) return 1;
        if (entries[r](1, one, pi, nullptr, 0.2, 1e-4, 100, pf, pf, pi, pf, pi, nullptr) != GADAPT_MESH_E_BADARG) return 1;
        if (entries[r](1, one, pi, pf, 0.0, 1e-4, 100, pf, pf, pi, pf, pi, nullptr) != GADAPT_MESH_E_BADARG) return 1;
        if (entries[r](1, one, pi, pf, 0.2, -1.0, 100, pf, pf, pi, pf, pi, nullptr) != GADAPT_MESH_E_BADARG) return 1;
        if (entries[r](1, one, pi, pf, 0.2, 1e-4, -1, pf, pf, pi, pf, pi, nullptr) != GADAPT_MESH_E_SIZE) return 1;
        if (entries[r](1, one, pi, pf, 0.2, 1e-4, GADAPT_MMPDE5_MAX_STEPS + 1, pf, pf, pi, pf, pi, nullptr) != GADAPT_MESH_E_SIZE) return 1;
        if (entries[r](1, one, pi, pf, 0.2, 0.0, GADAPT_MMPDE5_MAX_STEPS, pf, pf, pi, pf, pi, nullptr) != GADAPT_MESH_OK) return 1;
        calls += 8;
    }
    printf("%ld calls of the two entry points, every return code and launch geometry as expected\n", calls);
    return 0;
}
