// fem_topology.cpp - host build of the per-batch FEM topology (include/gadapt_fem.h).
//
// Interior numbering, the band of P_II in that numbering and the node -> incident-triangle CSR that
// every gather of the FEM kernels walks.  Built once per batch topology; the caller caches it.
#include <stdint.h>
#include <stdlib.h>
#include "gadapt_fem.h"

extern "C" int64_t gadapt_fem_topology_host(int B, const int32_t* node_off, const int32_t* tri_off, const int32_t* cells,
                                            const uint8_t* boundary, int32_t* meta, int32_t* node_mesh, int32_t* tri_mesh,
                                            int32_t* int_idx, int32_t* int_node, int32_t* nt_ptr, int32_t* nt_idx) {
    if (B <= 0 || !node_off || !tri_off || !cells || !boundary || !meta || !node_mesh || !tri_mesh || !int_idx || !int_node ||
        !nt_ptr || !nt_idx || node_off[0] != 0 || tri_off[0] != 0)
        return GADAPT_FEM_E_BADARG;
    for (int b = 0; b < B; ++b)
        if (node_off[b + 1] < node_off[b] || tri_off[b + 1] < tri_off[b]) return GADAPT_FEM_E_BADARG;
    const int32_t N = node_off[B], T = tri_off[B];
    for (int32_t i = 0; i <= N; ++i) nt_ptr[i] = 0;
    for (int b = 0; b < B; ++b) {
        for (int32_t v = node_off[b]; v < node_off[b + 1]; ++v) node_mesh[v] = b;
        for (int32_t t = tri_off[b]; t < tri_off[b + 1]; ++t) {
            tri_mesh[t] = b;
            for (int k = 0; k < 3; ++k) {
                const int32_t v = cells[3 * t + k];
                if (v < node_off[b] || v >= node_off[b + 1]) return GADAPT_FEM_E_RANGE;
                nt_ptr[v + 1]++;
            }
        }
    }
    for (int32_t i = 0; i < N; ++i) nt_ptr[i + 1] += nt_ptr[i];
    // triangles in increasing id, local vertices in increasing order: the order torch.where(cell_node_map == m) walks
    // (difFEM_2d.py:33), so sums over incident triangles run in the reference's order
    int32_t* fill = (int32_t*)malloc(sizeof(int32_t) * (N > 0 ? N : 1));
    if (!fill) return GADAPT_FEM_E_BADARG;
    for (int32_t i = 0; i < N; ++i) fill[i] = nt_ptr[i];
    for (int32_t t = 0; t < T; ++t)
        for (int k = 0; k < 3; ++k) nt_idx[fill[cells[3 * t + k]]++] = 4 * t + k;
    free(fill);

    int64_t band_off = 0;
    int32_t int_off = 0;
    for (int b = 0; b < B; ++b) {
        int32_t n_int = 0;
        for (int32_t v = node_off[b]; v < node_off[b + 1]; ++v) {
            if (boundary[v]) {
                int_idx[v] = -1;
            } else {
                int_idx[v] = n_int;
                int_node[int_off + n_int] = v;
                ++n_int;
            }
        }
        int32_t band = 0;
        for (int32_t t = tri_off[b]; t < tri_off[b + 1]; ++t)
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) {
                    const int32_t a = int_idx[cells[3 * t + i]], c = int_idx[cells[3 * t + j]];
                    if (a >= 0 && c >= 0 && abs(a - c) > band) band = abs(a - c);
                }
        int32_t* m = meta + (int64_t)b * GADAPT_FEM_META;
        m[GADAPT_FEM_M_NODE_OFF] = node_off[b];
        m[GADAPT_FEM_M_N_NODES] = node_off[b + 1] - node_off[b];
        m[GADAPT_FEM_M_TRI_OFF] = tri_off[b];
        m[GADAPT_FEM_M_N_TRIS] = tri_off[b + 1] - tri_off[b];
        m[GADAPT_FEM_M_INT_OFF] = int_off;
        m[GADAPT_FEM_M_N_INT] = n_int;
        m[GADAPT_FEM_M_BAND] = band;
        if (band_off > INT32_MAX) return GADAPT_FEM_E_BADARG;
        m[GADAPT_FEM_M_BAND_OFF] = (int32_t)band_off;
        band_off += (int64_t)n_int * (band + 1);
        int_off += n_int;
    }
    return band_off;
}

extern "C" int64_t gadapt_fem_factor_lds_bytes(int n_int, int band) {
    // band factor, right-hand side, and the (i, j) pair table of the rank-1 update (fem_kernels.hip: band_factor)
    return (int64_t)n_int * (band + 1) * 4 + (int64_t)n_int * 4 + (int64_t)band * (band + 1) / 2 * 4;
}
