// ma_host_sweep.cpp - the one host-side batch check of the nine Monge-Ampere entry points (mesh_csrc/ma_host.h: check_batch and
// the launch geometry) as a stand-alone host program for sanitizer builds.  It builds from this file and the headers alone: no
// kernel file, no kernel launched, no device needed.
//   hipcc --offload-arch=gfx950 -x hip -std=c++17 -g -Iinclude -Ig_adaptivity_amd/mesh_csrc -ffp-contract=off \
//       -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//       tools/ma_host_sweep.cpp -o build/ma_host_sweep
//   build/ma_host_sweep
// Descriptors live in heap buffers of exactly the size they need, so a read past a batch's last word is a heap overflow.
// Table descriptors (both routes' side limits) and Gaussian descriptors (the three side limits 24, 32, 81; ng in -1, 0, 8, 9) are
// swept as the last mesh of batches of 1 to 3; return codes, the thread count and the LDS bytes of every kernel the geometry
// serves are compared with this file's own arithmetic.  Prints the number of calls and exits 0, or says what was wrong and
// exits 1.
#include <limits.h>
#include <stdint.h>
#include <stdio.h>
#include <vector>

#include "gadapt_mesh.h"
#include "ma_host.h"

using namespace gadapt_ma;

static float dummy_f = 0.0f;
static int32_t dummy_i = 0;
static float* const pf = &dummy_f;                           // never dereferenced: nothing is launched
static int32_t* const pi = &dummy_i;

// the check as an entry point calls it, with the scalar arguments and pointers given
static int call(int max_side, bool table, int B, const int32_t* desc_host, const void* field, const void* mon, double cfl, double tol,
                int max_steps, Geometry* g) {
    return check_batch("sweep", max_side, max_side == SLOW_MAX_SIDE ? BAND_IN_LDS : ONE_WORKGROUP, table, B, desc_host, pi, field, mon,
                       cfl, tol, max_steps, pf, pf, pi, pf, pi, g);
}

// what the launch of the good batch below has to be given: its own arithmetic, not the header's
static bool geometry_ok(int max_side, bool table, int B, int N, const Geometry& g) {
    const int big = N > 11 || B == 1 ? N : 11, nodes = big * big, rounded = (nodes + 63) & ~63;
    const int threads = rounded < 1024 ? rounded : 1024;
    if (g.threads != threads || g.side != big) return false;
    const int64_t image = 8 * (int64_t)nodes;                // two fp32 images or one fp64 image
    if (table) return lane_lds_bytes(TABLE_HEAD, nodes) == 256 + image && strided_lds_bytes(TABLE_HEAD, nodes) == 256 + image &&
                      256 + image <= 65536;
    if (max_side == SLOW_MAX_SIDE) {
        const int64_t w = big - 2;
        const int64_t want = 4 * (6 * 16 + 64 + 4 + 6 * (int64_t)nodes + w * w * (w + 1) + w * w);
        return slow_lds_bytes(big) == want && want <= 65536;
    }
    const bool lane = max_side == LANE_MAX_SIDE;
    const int64_t ma = lane ? lane_lds_bytes(MA_HEAD, nodes) : strided_lds_bytes(MA_HEAD, nodes);
    const int64_t m2n = lane ? lane_lds_bytes(M2N_HEAD, nodes) : strided_lds_bytes(M2N_HEAD, nodes);
    return ma == 512 + image && m2n == 592 + image && m2n <= 65536;
}

int main() {
    const int ns[] = {INT_MIN, -1, 0, 2, 3, 8, 9, 23, 24, 25, 31, 32, 33, 80, 81, 82, 46341, INT_MAX};
    const int ts[] = {INT_MIN, -1, 0, 1, 2, 3, 1023, 1024, 1025, 46341, INT_MAX};
    const int ngs[] = {-1, 0, 8, 9};
    const int offs[] = {INT_MIN, -1, 0, 1, INT_MAX - 1024 * 1024 - 1, INT_MAX - 1024 * 1024, INT_MAX - 1024 * 1024 + 1, INT_MAX - 6561,
                        INT_MAX - 6560, INT_MAX - 4, INT_MAX - 3, INT_MAX};
    const int table_sides[2] = {LANE_MAX_SIDE, STRIDED_MAX_SIDE}, gauss_sides[3] = {SLOW_MAX_SIDE, LANE_MAX_SIDE, STRIDED_MAX_SIDE};
    if (SLOW_MAX_SIDE != 24 || LANE_MAX_SIDE != 32 || STRIDED_MAX_SIDE != 81 || MAX_TABLE_SIDE != 1024 || MAX_GAUSS != 8) return 1;
    long calls = 0;
    for (int pass = 0; pass < 2; ++pass) {                   // pass 0: tables (words 2, 3 = offset, T); pass 1: Gaussians (offset, ng)
        const bool table = pass == 0;
        for (int side : (table ? std::vector<int>(table_sides, table_sides + 2) : std::vector<int>(gauss_sides, gauss_sides + 3)))
        for (int B = 1; B <= 3; ++B)
        for (int N : ns) for (int noff : offs) for (int off : offs) {
            const std::vector<int> counts = table ? std::vector<int>(ts, ts + 11) : std::vector<int>(ngs, ngs + 4);
            for (int cnt : counts) for (int null_field = 0; null_field < (table ? 1 : 2); ++null_field) {
                std::vector<int32_t> desc((size_t)GADAPT_MA_DESC * B);
                for (int b = 0; b < B - 1; ++b) {            // good meshes first: the one under test is the last of the batch
                    desc[4 * b + GADAPT_MA_D_N] = 11, desc[4 * b + GADAPT_MA_D_NODE_OFF] = 121 * b;
                    desc[4 * b + 2] = table ? 81 * b : 2 * b, desc[4 * b + 3] = table ? 9 : 2;
                }
                int32_t* d = desc.data() + 4 * (B - 1);
                d[GADAPT_MA_D_N] = N, d[GADAPT_MA_D_NODE_OFF] = noff, d[2] = off, d[3] = cnt;
                const bool no_gauss = null_field == 1;       // a null Gaussian array is good only if no mesh has a Gaussian
                Geometry g = {-1, -1};
                const int rc = call(side, table, B, desc.data(), no_gauss ? nullptr : (const void*)pf, pf, 0.2, 1e-4, 100, &g);
                ++calls;
                int want;
                if (table) {
                    const bool bad = N < 3 || noff < 0 || off < 0;
                    const bool size = N > side || cnt < 2 || cnt > 1024 || (int64_t)noff + (int64_t)N * N > INT_MAX ||
                                      (int64_t)off + (int64_t)cnt * cnt > INT_MAX;
                    want = bad ? GADAPT_MESH_E_BADARG : size ? GADAPT_MESH_E_SIZE : GADAPT_MESH_OK;
                } else {
                    const bool bad = (no_gauss && B > 1) || N < 3 || noff < 0 || off < 0 || cnt < 0 || (cnt > 0 && no_gauss);
                    const bool size = N > side || cnt > 8 || (int64_t)noff + (int64_t)N * N > INT_MAX;
                    want = bad ? GADAPT_MESH_E_BADARG : size ? GADAPT_MESH_E_SIZE : GADAPT_MESH_OK;
                }
                if (rc != want) {
                    printf("pass %d side %d B %d N %d words %d / %d offset %d null %d: %d, expected %d\n", pass, side, B, N, off, cnt, noff,
                           null_field, rc, want);
                    return 1;
                }
                if (rc == GADAPT_MESH_OK && !geometry_ok(side, table, B, N, g)) {
                    printf("pass %d side %d B %d N %d: %d threads, largest side %d\n", pass, side, B, N, g.threads, g.side);
                    return 1;
                }
                if (rc != GADAPT_MESH_OK && (g.threads != -1 || g.side != -1)) { printf("geometry written on an error\n"); return 1; }
            }
        }
    }
    for (int pass = 0; pass < 2; ++pass) {                   // the scalar arguments and the null pointers
        const bool table = pass == 0;
        const int32_t one[4] = {11, 0, 0, table ? 9 : 2};
        Geometry g;
        if (call(32, table, 0, one, pf, pf, 0.2, 1e-4, 100, &g) != GADAPT_MESH_E_BADARG) return 1;
        if (call(32, table, 1, nullptr, pf, pf, 0.2, 1e-4, 100, &g) != GADAPT_MESH_E_BADARG) return 1;
        if (call(32, table, 1, one, table ? nullptr : pf, table ? pf : nullptr, 0.2, 1e-4, 100, &g) != GADAPT_MESH_E_BADARG) return 1;
        if (call(32, table, 1, one, pf, pf, 0.0, 1e-4, 100, &g) != GADAPT_MESH_E_BADARG) return 1;
        if (call(32, table, 1, one, pf, pf, 0.2, -1.0, 100, &g) != GADAPT_MESH_E_BADARG) return 1;
        if (call(32, table, 1, one, pf, pf, 0.2, 1e-4, -1, &g) != GADAPT_MESH_E_SIZE) return 1;
        if (call(32, table, 1, one, pf, pf, 0.2, 1e-4, GADAPT_MMPDE5_MAX_STEPS + 1, &g) != GADAPT_MESH_E_SIZE) return 1;
        if (call(32, table, 1, one, pf, pf, 0.2, 0.0, GADAPT_MMPDE5_MAX_STEPS, &g) != GADAPT_MESH_OK) return 1;
        calls += 8;
    }
    printf("%ld calls of the batch check, every return code and launch geometry as expected\n", calls);
    return 0;
}
