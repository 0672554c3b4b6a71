// cnn_plan_sweep.cpp - the size and check functions of the global CNN features (csrc/gadapt_cnn_plan.h, plain host C++) as a stand-alone
// host program for sanitizer builds:
//   clang++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Ig_adaptivity_amd/csrc tools/cnn_plan_sweep.cpp \
//       -o build/cnn_plan_sweep && build/cnn_plan_sweep
// Over every dim, image side 1..40 (both sides at dim 2), mid in {1, 3, 8, 16, 32, 64}, out in {3, 8} and 1..3 meshes it checks that a
// refusal is written within the caller's buffer (a heap buffer of exactly the size passed), that what is not refused fits the LDS
// budget, that the parameter and workspace offsets tile their buffers without a gap or overlap, and that the launch sizes are whole
// waves within 1024 threads.  Prints the number of shapes and exits 0, or says what was wrong and exits 1.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "gadapt_cnn_plan.h"

int main() {
    const int widths[] = {1, 3, 8, 16, 32, 64};
    long shapes = 0, taken = 0;
    for (int dim = 0; dim <= 3; ++dim)
    for (int n0 = 0; n0 <= (dim == 2 ? 40 : 2); ++n0)
    for (int n1 = 0; n1 <= 40; ++n1)
    for (int mid : widths) for (int out : {3, 8})
    for (int B = 0; B <= 3; ++B)
    for (int images = 2; images <= 3; ++images) {
        ++shapes;
        std::vector<char> msg(96);                               // shorter than the longest message: snprintf must cut it, not overrun
        const char* why = cnn_plan::refuse("sweep", B, dim, n0, n1, mid, out, images, msg.data(), msg.size());
        if (why) {
            if (why != msg.data() || strlen(why) >= msg.size() || strncmp(why, "sweep: ", 7)) { printf("bad refusal text\n"); return 1; }
            continue;
        }
        ++taken;
        if (!cnn_plan::sizes_ok(dim, n0, n1, mid, out) || B < 1) { printf("took bad sizes\n"); return 1; }
        const int64_t lds = images == 2 ? cnn_plan::forward_lds_bytes(n0, n1, mid, out) : cnn_plan::backward_lds_bytes(n0, n1, mid, out);
        if (lds <= 0 || lds > GADAPT_CNN_LDS_BUDGET || lds != 4 * (images * cnn_plan::image_floats(n0, n1, mid, out) + cnn_plan::pixels(n0, n1))) {
            printf("LDS of %lld bytes taken at dim %d, %d x %d, %d / %d\n", (long long)lds, dim, n0, n1, mid, out); return 1;
        }
        // every parameter and every saved activation lies in exactly one layer's slice
        std::vector<uint8_t> params(cnn_plan::param_floats(dim, mid, out)), acts(cnn_plan::workspace_floats(B, n0, n1, mid, out));
        for (int l = 0; l < GADAPT_CNN_LAYERS; ++l) {
            const int64_t po = cnn_plan::param_offset(l, dim, mid, out), pn = cnn_plan::weight_floats(l, dim, mid, out) + cnn_plan::c_out(l, mid, out);
            for (int64_t i = 0; i < pn; ++i) ++params.at(po + i);
            const int64_t ao = cnn_plan::acts_offset(l, B, n0, n1, mid, out), an = (int64_t)B * cnn_plan::c_out(l, mid, out) * cnn_plan::pixels(n0, n1);
            for (int64_t i = 0; i < an; ++i) ++acts.at(ao + i);
        }
        for (uint8_t c : params) if (c != 1) { printf("parameter slices overlap or leave a gap\n"); return 1; }
        for (uint8_t c : acts) if (c != 1) { printf("activation slices overlap or leave a gap\n"); return 1; }
        for (int nt : {cnn_plan::forward_threads(n0, n1, mid, out), cnn_plan::backward_threads(dim, n0, n1, mid, out)})
            if (nt < 256 || nt > 1024 || nt % 256) { printf("workgroup of %d threads\n", nt); return 1; }
    }
    printf("%ld shapes, %ld taken\n", shapes, taken);
    return 0;
}
