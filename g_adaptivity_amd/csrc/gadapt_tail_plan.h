// gadapt_tail_plan.h - entry map of the narrow route's spread step tail (step_tail_narrow_spread_kernel, gadapt_small.inc; hidden 64): one
// definition for the kernel, its launcher and the host copy that the CPU tests call (gadapt_narrow_tail_*_host, csr_build.cpp).
//
// The flat bucket [Wq | bq | Wk | bk] has 2 * 64 * 64 + 2 * 64 = 8320 entries.  A parameter workgroup owns GADAPT_NARROW_TAIL_ROWS
// consecutive rows r of it - Wq[r][0..63], bq[r], Wk[r][0..63], bk[r]: 130 entries per row - so the chain rule of its entries
//     d Wq[r][c] = sum_o Wk[r][o] dA[o][c]      d Wk[r][o] = sum_c Wq[r][c] dA[o][c] + bq[r] dp0[o]      d bq[r] = sum_o Wk[r][o] dp0[o]
// reads only parameters the same workgroup owns, and no workgroup reads what another writes (step_tail_kernel's rule).  The last
// workgroup may own fewer rows.  Within a workgroup of nr rows the entries are numbered l = 0 .. 130 nr - 1: its Wq rows (64 nr,
// contiguous in the bucket), its Wk rows (64 nr, contiguous), its bq entries, its bk entries; thread t holds l = t, t + T, ... (slots).
#ifndef GADAPT_TAIL_PLAN_H
#define GADAPT_TAIL_PLAN_H

#include <stdint.h>

#ifndef GADAPT_NARROW_TAIL_ROWS
#define GADAPT_NARROW_TAIL_ROWS 1       /* rows of the bucket a parameter workgroup owns (docs/measurements.md: the geometries tried) */
#endif
#ifndef GADAPT_NARROW_TAIL_THREADS
#define GADAPT_NARROW_TAIL_THREADS 256  /* threads of a workgroup: a multiple of 256 (the first 256 sum the slab) */
#endif
#define GADAPT_NARROW_TAIL_C 64
#define GADAPT_NARROW_TAIL_ROW_ENTRIES (2 * GADAPT_NARROW_TAIL_C + 2)

#ifdef __HIPCC__
#define GADAPT_TAIL_FN __host__ __device__ static inline constexpr
#elif defined(__cplusplus)
#define GADAPT_TAIL_FN static inline constexpr
#else
#define GADAPT_TAIL_FN static inline
#endif

// parameter workgroups (each takes one ticket), rows of workgroup wg, slots per thread
GADAPT_TAIL_FN int gadapt_narrow_tail_wgs(void) { return (GADAPT_NARROW_TAIL_C + GADAPT_NARROW_TAIL_ROWS - 1) / GADAPT_NARROW_TAIL_ROWS; }
GADAPT_TAIL_FN int gadapt_narrow_tail_rows_of(int wg) {
    return (wg + 1) * GADAPT_NARROW_TAIL_ROWS <= GADAPT_NARROW_TAIL_C ? GADAPT_NARROW_TAIL_ROWS : GADAPT_NARROW_TAIL_C - wg * GADAPT_NARROW_TAIL_ROWS;
}
GADAPT_TAIL_FN int gadapt_narrow_tail_slots(void) {
    return (GADAPT_NARROW_TAIL_ROWS * GADAPT_NARROW_TAIL_ROW_ENTRIES + GADAPT_NARROW_TAIL_THREADS - 1) / GADAPT_NARROW_TAIL_THREADS;
}
// workgroups of the launch (the loss workgroup, when there are loss partials, comes last and takes no ticket) and tickets taken
GADAPT_TAIL_FN int gadapt_narrow_tail_grid(int has_loss) { return gadapt_narrow_tail_wgs() + (has_loss ? 1 : 0); }
GADAPT_TAIL_FN int gadapt_narrow_tail_tickets(int has_loss) { return (void)has_loss, gadapt_narrow_tail_wgs(); }

// (workgroup, thread, slot) -> its entry: e = index into the flat bucket (-1: the slot holds nothing), ri = row within the workgroup
// (row r = wg * ROWS + ri), k = place in the row: 0..63 Wq[r][k], 64 bq[r], 65..128 Wk[r][k - 65], 129 bk[r]
struct gadapt_tail_entry { int e, ri, k; };
GADAPT_TAIL_FN struct gadapt_tail_entry gadapt_narrow_tail_entry(int wg, int thread, int slot) {
    const int C = GADAPT_NARROW_TAIL_C, c2 = C * C, nr = gadapt_narrow_tail_rows_of(wg), r0 = wg * GADAPT_NARROW_TAIL_ROWS;
    const int l = slot * GADAPT_NARROW_TAIL_THREADS + thread;
    struct gadapt_tail_entry t = {-1, 0, 0};
    if (l < nr * C) { t.ri = l / C; t.k = l % C; t.e = (r0 + t.ri) * C + t.k; }
    else if (l < 2 * nr * C) { const int f = l - nr * C; t.ri = f / C; t.k = C + 1 + f % C; t.e = c2 + C + (r0 + t.ri) * C + f % C; }
    else if (l < 2 * nr * C + nr) { t.ri = l - 2 * nr * C; t.k = C; t.e = c2 + r0 + t.ri; }
    else if (l < 2 * nr * C + 2 * nr) { t.ri = l - 2 * nr * C - nr; t.k = 2 * C + 1; t.e = 2 * c2 + C + r0 + t.ri; }
    return t;
}
// entry e of the flat bucket -> the (workgroup, thread, slot) that owns it
struct gadapt_tail_owner { int wg, thread, slot; };
GADAPT_TAIL_FN struct gadapt_tail_owner gadapt_narrow_tail_owner(int e) {
    const int C = GADAPT_NARROW_TAIL_C, c2 = C * C;
    int r = 0, l = 0;
    if (e < c2) r = e / C; else if (e < c2 + C) r = e - c2; else if (e < 2 * c2 + C) r = (e - c2 - C) / C; else r = e - 2 * c2 - C;
    const int wg = r / GADAPT_NARROW_TAIL_ROWS, ri = r % GADAPT_NARROW_TAIL_ROWS, nr = gadapt_narrow_tail_rows_of(wg);
    if (e < c2) l = ri * C + e % C; else if (e < c2 + C) l = 2 * nr * C + ri; else if (e < 2 * c2 + C) l = nr * C + ri * C + (e - c2 - C) % C;
    else l = 2 * nr * C + nr + ri;
    struct gadapt_tail_owner o = {wg, l % GADAPT_NARROW_TAIL_THREADS, l / GADAPT_NARROW_TAIL_THREADS};
    return o;
}

#endif  // GADAPT_TAIL_PLAN_H
