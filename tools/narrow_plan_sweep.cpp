// narrow_plan_sweep.cpp - the enumeration of tests/test_host_narrow_step_plan.py (a) through gadapt_narrow_step_plan_host, as a
// stand-alone host program for sanitizer builds: every plan is written into a heap buffer of exactly the size it needs, read back, and
// its buffer offsets are checked against the caller's buffers.  csrc/gadapt_narrow_plan.h and csrc/csr_build.cpp are plain host C++:
//   clang++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ig_adaptivity_amd/csrc \
//       tools/narrow_plan_sweep.cpp g_adaptivity_amd/csrc/csr_build.cpp -o build/narrow_plan_sweep && build/narrow_plan_sweep
// Prints the number of plans and exits 0, or says what was wrong and exits 1.
#include <stdint.h>
#include <stdio.h>
#include <vector>
#include "gadapt_hip.h"
#include "gadapt_narrow_plan.h"

static int slab_rows_64(int64_t n) {                             // gadapt_backward_slab_rows at hidden 64: 64-node tiles, a multiple of 8, 8 .. 512
    int64_t g = ((n + 63) / 64 + 7) & ~(int64_t)7;
    return (int)(g > 512 ? 512 : (g < 8 ? 8 : g));
}

int main() {
    const int64_t sizes[] = {1, 255, 256, 257, 511, 512, 513, 64 * 256 - 1, 64 * 256, 64 * 512 - 1, 64 * 512, 131072, 131073};
    const int halos[] = {0, 32, 64}, c = 64;
    long plans = 0;
    for (int L = 1; L <= 8; ++L)
    for (int64_t n : sizes) {
    const int words = GADAPT_NARROW_PLAN_HEAD + GADAPT_NARROW_LAUNCH_WORDS * 3 * L;     // always holds a plan of L layers
    std::vector<int32_t> big(words);
    for (int bound = 0; bound < 2; ++bound)
    for (int64_t de = -1; de <= 1; ++de)
    for (int ht : halos) for (int hs : halos)
    for (int kmax = 8; kmax <= 9; ++kmax)
    for (int flags = 0; flags < 128; ++flags)
    for (int sw = 0; sw < 24; ++sw) {
        const int64_t e0 = (int64_t)(c - (bound ? 8 : 4)) * n / 2 + de, e = e0 < 0 ? 0 : e0;
        const int64_t facts[GADAPT_NARROW_FACTS] = {n, e, c, L, 1, ht, hs, kmax, slab_rows_64(n), (n + 511) / 512 * 8 <= 4096, 1, 1, 1, 1, 1,
                                                    flags & 1, (flags >> 1) & 1, (flags >> 2) & 1, (flags >> 3) & 1, (flags >> 4) & 1, (flags >> 5) & 1,
                                                    (flags >> 6) & 1};
        const int32_t switches[4] = {sw % 3, (sw / 3) & 1, (sw / 6) & 1, (sw / 12) & 1};
        const int need = gadapt_narrow_step_plan_host(facts, switches, big.data(), words);
        if (need < GADAPT_NARROW_PLAN_HEAD || need > words) { printf("plan of %d words at L = %d\n", need, L); return 1; }
        std::vector<int32_t> p(need);                            // exactly as long as the plan: a word too many is a heap overflow
        if (gadapt_narrow_step_plan_host(facts, switches, p.data(), need) != need) { printf("exact cap refused\n"); return 1; }
        if (gadapt_narrow_step_plan_host(facts, switches, p.data(), need - 1) != GADAPT_E_BADARG) { printf("cap - 1 accepted\n"); return 1; }
        const int32_t *g = &p[12], *d = &p[14], *ed = &p[16];
        for (int i = 0; i < p[1] + p[2]; ++i) {
            const int32_t* r = &p[GADAPT_NARROW_PLAN_HEAD + GADAPT_NARROW_LAUNCH_WORDS * i];
            bool ok = r[0] >= 0 && r[0] <= 7 && r[1] >= 0 && r[1] < L && r[2] >= 1 && r[1] + (i < p[1] ? r[2] : 0) <= L;
            for (int k = 3; k <= 8; ++k) ok = ok && r[k] >= -1 && r[k] <= 1;
            for (int k = 3; k <= 4 && ok; ++k) ok = r[k] < 0 || (int64_t)g[r[k]] + 4 * n <= 2 * n * c;
            for (int k = 7; k <= 8 && ok; ++k) ok = r[k] < 0 || (int64_t)d[r[k]] + 4 * n <= n * c;
            for (int k = 5; k <= 6 && ok; ++k) ok = r[k] < 0 || (r[k] == 0 ? ed[0] == 0 : (int64_t)ed[1] + 2 * e <= n * c);
            if (!ok) { printf("launch %d of the plan at n = %lld, e = %lld, L = %d, flags %d, switches %d: bad record\n", i, (long long)n, (long long)e, L, flags, sw); return 1; }
        }
        ++plans;
    }
    }
    printf("%ld plans\n", plans);
    return 0;
}
