// mmpde5_kernels.hip - batched MMPDE5 target-mesh generation (include/gadapt_mesh.h).
//
// One workgroup per mesh, the whole pseudo-time loop inside the launch.  The monitor does not move with the mesh, so every
// node's stencil is four constant coefficients; they stay in registers with the node's coordinates, and the stage values go
// through two LDS images that alternate, so that a stage needs one barrier: a stage writes image s & 1 and reads its
// neighbours there, and the image it overwrites was last read two barriers ago.  The wave sums of the update measure ride
// on the barrier of the next step's first stage (two slots, by step parity), every lane adds them in the same order and
// takes the same exit.
//
// One lane per node, as many waves as the mesh needs (up to 16).  One wave per mesh with several nodes per lane and no
// workgroup barrier was built and measured too: slower on a single mesh (4.35 against 1.16 ms for 1000 steps at 23 x 23,
// 0.87 against 0.72 at 11 x 11) and on full batches (4.49 against 2.94 ms for 1024 meshes of 23 x 23), so it was deleted
// (docs/measurements.md).  A mesh's thread count follows from its own node count, so its arithmetic and the order of its
// reduction do not depend on the batch it is launched in; waves beyond a mesh's own only keep the barriers company.
//
// route='strided' (mmpde5_strided_kernel, gadapt_mmpde5_batch_strided): the same arithmetic with K = ceil(nodes / T) nodes per
// lane, T = min(mmpde5_threads(nodes), 1024), for 2-D meshes up to 81 x 81 (K <= 7).  Lane tid owns nodes tid + k * T, so
// neighbouring lanes read neighbouring LDS words; the four stencil constants, x, y, the stage value and the RK4 accumulator
// of every owned node stay in registers (K is a template parameter, every per-node array is indexed by constants), the two
// images stay in LDS (105 104 B at 81 x 81: the launch raises the kernel's dynamic-LDS limit once per device).  A lane adds
// |dx| + |dy| of its nodes in increasing k, then wave_sum, then the waves in increasing order: for K = 1 this is
// mmpde5_kernel's code operation for operation, so a mesh of at most 1024 nodes gives the same bits on both routes.  One
// kernel holds all K (a mesh picks its own by a uniform switch), so its register count is that of K = 7: 116 VGPRs, no AGPRs,
// 70 SGPRs, no scratch (hipcc -Rpass-analysis=kernel-resource-usage, gfx950, 1024 lanes = 4 waves per SIMD = 128 registers).
// Built with the switch pinned to one K, the instantiations K = 1..7 take 32, 48, 60, 74, 88, 102 and 116 VGPRs, none with
// scratch.  Two things keep it there, both marked in the code: the LDS addresses of a slot are rebuilt in every stage and not
// hoisted out of the loop, and the x and y halves of a slot are not fused into packed fp32 pairs.
//
// Built without FMA contraction (Makefile and the pragma below): the stopping step of the fp32 iteration depends on the
// rounding of increments near half an ulp, and the parity bars are stated against uncontracted fp32 arithmetic.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "gadapt_mesh.h"
#include "mesh_common.h"

#pragma clang fp contract(off)

using namespace gadapt_mesh_shared;                      // g_err, mesh_fail, dpp_move, wave_sum

namespace {

constexpr int MAX_NODES = GADAPT_MMPDE5_MAX_NODES;
constexpr int MAX_WAVES = MAX_NODES / 64;

// Threads of a mesh: one lane per node, whole waves.
__host__ __device__ inline int mmpde5_threads(int nodes) { return (nodes + 63) & ~63; }

// red[2][MAX_WAVES] in front, then the two images of (X, Y), each MAX of the batch's nodes long
__host__ __device__ inline int64_t mmpde5_lds_floats(int nodes) { return 2 * MAX_WAVES + 4 * (int64_t)nodes; }

struct Params {
    float h, h6, tol, stiff;
    int tol_zero, max_steps;
    double tau;
};

// The right-hand side of one coordinate at one node: `u` is the node's own stage value, the neighbours come from the image.
template <int DIM>
__device__ inline float rhs(const float* __restrict__ img, float u, int c, int oi, int oj, float aE, float aW, float aS, float cf) {
    const float a1 = aE * (img[c + oi] - u) - aW * (u - img[c - oi]);
    if (DIM == 1) return a1 * cf;
    const float a2 = aE * (img[c + oj] - u) - aS * (u - img[c - oj]);
    return (a1 + a2) * cf;
}

template <int DIM>
__device__ void mmpde5_run(const int32_t* __restrict__ d, const float* __restrict__ x0, const float* __restrict__ y0,
                           const float* __restrict__ ms, const float* __restrict__ m2, const Params p, float* __restrict__ xo,
                           float* __restrict__ yo, int32_t* __restrict__ steps, float* __restrict__ measure,
                           int32_t* __restrict__ status, float* lds) {
    const int N = d[GADAPT_MMPDE5_D_N], noff = d[GADAPT_MMPDE5_D_NODE_OFF], coff = d[GADAPT_MMPDE5_D_CELL_OFF];
    const int nodes = DIM == 2 ? N * N : N;
    const int T = mmpde5_threads(nodes), nw = T >> 6;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    float* red = lds;
    float* imgX[2] = {lds + 2 * MAX_WAVES, lds + 2 * MAX_WAVES + 2 * nodes};
    float* imgY[2] = {imgX[0] + nodes, imgX[1] + nodes};

    float x, y, aE, aW, aS, cf;
    int c, oi, oj;
    bool own;
    const double dxi = 1.0 / (double)(N - 1);
    {
        own = tid < nodes;
        c = own ? tid : 0;
        bool inner;
        int cell, cellW, cellS = 0;
        if (DIM == 2) {
            const int i = c / N, j = c - i * N;
            inner = own && i > 0 && i < N - 1 && j > 0 && j < N - 1;
            cell = i * (N - 1) + j, cellW = cell - (N - 1), cellS = cell - 1;
            oi = inner ? N : 0, oj = inner ? 1 : 0;
        } else {
            inner = own && c > 0 && c < N - 1;
            cell = c, cellW = cell - 1;
            oi = inner ? 1 : 0, oj = 0;
        }
        aE = inner ? ms[coff + cell] : 0.0f;
        aW = inner ? ms[coff + cellW] : 0.0f;
        aS = (DIM == 2 && inner) ? ms[coff + cellS] : 0.0f;
        cf = inner ? (float)(1.0 / (dxi * dxi * p.tau * (double)m2[noff + c])) : 0.0f;
        x = own ? x0[noff + c] : 0.0f;
        y = (DIM == 2 && own) ? y0[noff + c] : 0.0f;
        if (own) {
            imgX[0][c] = x;
            if (DIM == 2) imgY[0][c] = y;
        }
    }

    int j = 0;
    float meas = 1.0f;                                   // the reference's starting value: tol >= 1 takes no step
    for (;;) {
        __syncthreads();                                 // image 0 holds the coordinates, red[j & 1] the wave sums of step j
        if (j > 0) {
            meas = red[(j & 1) * MAX_WAVES];
            for (int w = 1; w < nw; ++w) meas = meas + red[(j & 1) * MAX_WAVES + w];
        }
        // written so that a NaN measure ends the loop; with tol == 0 only the step count does
        if (!(j < p.max_steps && (p.tol_zero || meas > p.tol) && !(meas > p.stiff))) break;
        ++j;

        float sx, sy = 0.0f, kx, ky = 0.0f, ax, ay = 0.0f;
        ax = rhs<DIM>(imgX[0], x, c, oi, oj, aE, aW, aS, cf);          // k1 at the coordinates
        sx = x + (p.h * ax) * 0.5f;
        if (DIM == 2) {
            ay = rhs<DIM>(imgY[0], y, c, oi, oj, aE, aW, aS, cf);
            sy = y + (p.h * ay) * 0.5f;
        }
        if (own) {
            imgX[1][c] = sx;
            if (DIM == 2) imgY[1][c] = sy;
        }
        __syncthreads();
        kx = rhs<DIM>(imgX[1], sx, c, oi, oj, aE, aW, aS, cf);         // k2
        if (DIM == 2) ky = rhs<DIM>(imgY[1], sy, c, oi, oj, aE, aW, aS, cf);
        ax = ax + 2.0f * kx;
        sx = x + (p.h * kx) * 0.5f;
        if (DIM == 2) {
            ay = ay + 2.0f * ky;
            sy = y + (p.h * ky) * 0.5f;
        }
        if (own) {
            imgX[0][c] = sx;
            if (DIM == 2) imgY[0][c] = sy;
        }
        __syncthreads();
        kx = rhs<DIM>(imgX[0], sx, c, oi, oj, aE, aW, aS, cf);         // k3
        if (DIM == 2) ky = rhs<DIM>(imgY[0], sy, c, oi, oj, aE, aW, aS, cf);
        ax = ax + 2.0f * kx;
        sx = x + p.h * kx;
        if (DIM == 2) {
            ay = ay + 2.0f * ky;
            sy = y + p.h * ky;
        }
        if (own) {
            imgX[1][c] = sx;
            if (DIM == 2) imgY[1][c] = sy;
        }
        __syncthreads();
        kx = rhs<DIM>(imgX[1], sx, c, oi, oj, aE, aW, aS, cf);         // k4, the new coordinates, this lane's share of the measure
        if (DIM == 2) ky = rhs<DIM>(imgY[1], sy, c, oi, oj, aE, aW, aS, cf);
        const float xn = x + p.h6 * (ax + kx);
        float part = fabsf(xn - x);
        x = xn;
        if (DIM == 2) {
            const float yn = y + p.h6 * (ay + ky);
            part = part + fabsf(yn - y);
            y = yn;
        }
        if (own) {                                       // image 0 was last read before the barrier above
            imgX[0][c] = x;
            if (DIM == 2) imgY[0][c] = y;
        }
        const float wsum = wave_sum(part);
        if (lane == 0 && wave < nw) red[(j & 1) * MAX_WAVES + wave] = wsum;
    }

    if (own) {
        xo[noff + c] = x;
        if (DIM == 2) yo[noff + c] = y;
    }
    if (tid == 0) {
        *steps = j;
        *measure = meas;
        const bool finite = meas - meas == 0.0f;
        *status = (!finite || meas > p.stiff) ? GADAPT_MMPDE5_STIFF
                  : ((p.tol_zero || meas > p.tol) ? GADAPT_MMPDE5_CAP : GADAPT_MMPDE5_CONVERGED);
    }
}

__global__ __launch_bounds__(MAX_NODES) void mmpde5_kernel(const int32_t* __restrict__ desc, const float* __restrict__ x0,
                                                          const float* __restrict__ y0, const float* __restrict__ ms,
                                                          const float* __restrict__ m2, const double* __restrict__ step,
                                                          double tau, float tol, float stiff, int tol_zero, int max_steps,
                                                          float* __restrict__ xo, float* __restrict__ yo,
                                                          int32_t* __restrict__ steps, float* __restrict__ measure,
                                                          int32_t* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int b = blockIdx.x;
    const int32_t* d = desc + GADAPT_MMPDE5_DESC * b;
    const double h = step[b];
    // the reference multiplies fp32 tensors by the Python floats h and h / 6: each rounded to fp32 once
    const Params p{(float)h, (float)(h / 6.0), tol, stiff, tol_zero, max_steps, tau};
    if (d[GADAPT_MMPDE5_D_DIM] == 2)
        mmpde5_run<2>(d, x0, y0, ms, m2, p, xo, yo, steps + b, measure + b, status + b, lds);
    else
        mmpde5_run<1>(d, x0, y0, ms, m2, p, xo, yo, steps + b, measure + b, status + b, lds);
}

// ---------------------------------------------------------------------------------------------------------------------
// route='strided': K nodes per lane
constexpr int STRIDED_MAX_SIDE = 81;
constexpr int STRIDED_MAX_NODES = STRIDED_MAX_SIDE * STRIDED_MAX_SIDE;
constexpr int STRIDED_MAX_K = (STRIDED_MAX_NODES + MAX_NODES - 1) / MAX_NODES;
static_assert(STRIDED_MAX_K == 7, "mmpde5_strided_kernel dispatches K = 1..7");

__host__ __device__ inline int strided_threads(int nodes) {
    const int t = mmpde5_threads(nodes);
    return t < MAX_NODES ? t : MAX_NODES;
}

template <int DIM, int K>
__device__ void mmpde5_run_strided(const int32_t* __restrict__ d, const float* __restrict__ x0, const float* __restrict__ y0,
                                   const float* __restrict__ ms, const float* __restrict__ m2, const Params p,
                                   float* __restrict__ xo, float* __restrict__ yo, int32_t* __restrict__ steps,
                                   float* __restrict__ measure, int32_t* __restrict__ status, float* lds) {
    const int N = d[GADAPT_MMPDE5_D_N], noff = d[GADAPT_MMPDE5_D_NODE_OFF], coff = d[GADAPT_MMPDE5_D_CELL_OFF];
    const int nodes = DIM == 2 ? N * N : N;
    const int T = strided_threads(nodes), nw = T >> 6;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    float* red = lds;
    float* imgX[2] = {lds + 2 * MAX_WAVES, lds + 2 * MAX_WAVES + 2 * nodes};
    float* imgY[2] = {imgX[0] + nodes, imgX[1] + nodes};

    // bit k of `own` / `inner`: slot k holds a node / an interior node.  Node and neighbour offsets are rebuilt from the
    // two masks where they are used, so that they need not live in registers across the loop.
    float x[K], y[K], aE[K], aW[K], aS[K], cf[K];
    unsigned own = 0, inner = 0;
    const double dxi = 1.0 / (double)(N - 1);
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int idx = tid + k * T;
        const bool o = tid < T && idx < nodes;
        const int c = o ? idx : 0;
        bool in;
        int cell, cellW, cellS = 0;
        if (DIM == 2) {
            const int i = c / N, jj = c - i * N;
            in = o && i > 0 && i < N - 1 && jj > 0 && jj < N - 1;
            cell = i * (N - 1) + jj, cellW = cell - (N - 1), cellS = cell - 1;
        } else {
            in = o && c > 0 && c < N - 1;
            cell = c, cellW = cell - 1;
        }
        aE[k] = in ? ms[coff + cell] : 0.0f;
        aW[k] = in ? ms[coff + cellW] : 0.0f;
        aS[k] = (DIM == 2 && in) ? ms[coff + cellS] : 0.0f;
        cf[k] = in ? (float)(1.0 / (dxi * dxi * p.tau * (double)m2[noff + c])) : 0.0f;
        x[k] = o ? x0[noff + c] : 0.0f;
        y[k] = (DIM == 2 && o) ? y0[noff + c] : 0.0f;
        if (o) {
            imgX[0][c] = x[k];
            if (DIM == 2) imgY[0][c] = y[k];
        }
        own |= (unsigned)o << k;
        inner |= (unsigned)in << k;
    }
    // STRIDED_STAGE hands the compiler copies of tid and the masks that it cannot prove loop-invariant: hoisted out of the
    // pseudo-time loop, the 20 LDS addresses of every slot would cost more registers than the state itself (scratch from K = 4).
    int tv = tid;
    unsigned ov = own, iv = inner;
#define STRIDED_STAGE() asm volatile("" : "+v"(tv), "+v"(ov), "+v"(iv))
    // STRIDED_AFTER_X makes the y half of a slot depend on its x half, so that the two are not fused into packed fp32 pairs:
    // the pairs want every stencil constant twice, 28 registers more at K = 7.
#define STRIDED_AFTER_X(vx, vy) asm volatile("" : "+v"(vx), "+v"(vy))
#define STRIDED_SLOT(k)                                             \
    const bool o = (ov >> (k)) & 1u, in = (iv >> (k)) & 1u;         \
    const int c = o ? tv + (k) * T : 0;                             \
    const int oi = in ? (DIM == 2 ? N : 1) : 0, oj = (DIM == 2 && in) ? 1 : 0

    int j = 0;
    float meas = 1.0f;
    for (;;) {
        __syncthreads();                                 // image 0 holds the coordinates, red[j & 1] the wave sums of step j
        if (j > 0) {
            meas = red[(j & 1) * MAX_WAVES];
            for (int w = 1; w < nw; ++w) meas = meas + red[(j & 1) * MAX_WAVES + w];
        }
        if (!(j < p.max_steps && (p.tol_zero || meas > p.tol) && !(meas > p.stiff))) break;
        ++j;

        float sx[K], sy[K], ax[K], ay[K];
        STRIDED_STAGE();
#pragma unroll
        for (int k = 0; k < K; ++k) {                    // k1 at the coordinates
            STRIDED_SLOT(k);
            ax[k] = rhs<DIM>(imgX[0], x[k], c, oi, oj, aE[k], aW[k], aS[k], cf[k]);
            sx[k] = x[k] + (p.h * ax[k]) * 0.5f;
            if (DIM == 2) {
                float u = y[k];
                STRIDED_AFTER_X(sx[k], u);
                ay[k] = rhs<DIM>(imgY[0], u, c, oi, oj, aE[k], aW[k], aS[k], cf[k]);
                sy[k] = y[k] + (p.h * ay[k]) * 0.5f;
            }
            if (o) {
                imgX[1][c] = sx[k];
                if (DIM == 2) imgY[1][c] = sy[k];
            }
        }
        __syncthreads();
        STRIDED_STAGE();
#pragma unroll
        for (int k = 0; k < K; ++k) {                    // k2
            STRIDED_SLOT(k);
            const float kx = rhs<DIM>(imgX[1], sx[k], c, oi, oj, aE[k], aW[k], aS[k], cf[k]);
            ax[k] = ax[k] + 2.0f * kx;
            sx[k] = x[k] + (p.h * kx) * 0.5f;
            if (DIM == 2) {
                STRIDED_AFTER_X(sx[k], sy[k]);
                const float ky = rhs<DIM>(imgY[1], sy[k], c, oi, oj, aE[k], aW[k], aS[k], cf[k]);
                ay[k] = ay[k] + 2.0f * ky;
                sy[k] = y[k] + (p.h * ky) * 0.5f;
            }
            if (o) {
                imgX[0][c] = sx[k];
                if (DIM == 2) imgY[0][c] = sy[k];
            }
        }
        __syncthreads();
        STRIDED_STAGE();
#pragma unroll
        for (int k = 0; k < K; ++k) {                    // k3
            STRIDED_SLOT(k);
            const float kx = rhs<DIM>(imgX[0], sx[k], c, oi, oj, aE[k], aW[k], aS[k], cf[k]);
            ax[k] = ax[k] + 2.0f * kx;
            sx[k] = x[k] + p.h * kx;
            if (DIM == 2) {
                STRIDED_AFTER_X(sx[k], sy[k]);
                const float ky = rhs<DIM>(imgY[0], sy[k], c, oi, oj, aE[k], aW[k], aS[k], cf[k]);
                ay[k] = ay[k] + 2.0f * ky;
                sy[k] = y[k] + p.h * ky;
            }
            if (o) {
                imgX[1][c] = sx[k];
                if (DIM == 2) imgY[1][c] = sy[k];
            }
        }
        __syncthreads();
        float part = 0.0f;
        STRIDED_STAGE();
#pragma unroll
        for (int k = 0; k < K; ++k) {                    // k4, the new coordinates, this lane's share of the measure
            STRIDED_SLOT(k);
            const float kx = rhs<DIM>(imgX[1], sx[k], c, oi, oj, aE[k], aW[k], aS[k], cf[k]);
            const float xn = x[k] + p.h6 * (ax[k] + kx);
            float node = fabsf(xn - x[k]);
            x[k] = xn;
            if (DIM == 2) {
                STRIDED_AFTER_X(x[k], sy[k]);
                const float ky = rhs<DIM>(imgY[1], sy[k], c, oi, oj, aE[k], aW[k], aS[k], cf[k]);
                const float yn = y[k] + p.h6 * (ay[k] + ky);
                node = node + fabsf(yn - y[k]);
                y[k] = yn;
            }
            part = k == 0 ? node : part + node;          // a lane's nodes in increasing k
            if (o) {                                     // image 0 was last read before the barrier above
                imgX[0][c] = x[k];
                if (DIM == 2) imgY[0][c] = y[k];
            }
        }
        const float wsum = wave_sum(part);
        if (lane == 0 && wave < nw) red[(j & 1) * MAX_WAVES + wave] = wsum;
    }

#pragma unroll
    for (int k = 0; k < K; ++k) {
        STRIDED_SLOT(k);
        if (o) {
            xo[noff + c] = x[k];
            if (DIM == 2) yo[noff + c] = y[k];
        }
    }
#undef STRIDED_SLOT
#undef STRIDED_STAGE
#undef STRIDED_AFTER_X
    if (tid == 0) {
        *steps = j;
        *measure = meas;
        const bool finite = meas - meas == 0.0f;
        *status = (!finite || meas > p.stiff) ? GADAPT_MMPDE5_STIFF
                  : ((p.tol_zero || meas > p.tol) ? GADAPT_MMPDE5_CAP : GADAPT_MMPDE5_CONVERGED);
    }
}

__global__ __launch_bounds__(MAX_NODES) void mmpde5_strided_kernel(const int32_t* __restrict__ desc, const float* __restrict__ x0,
                                                                  const float* __restrict__ y0, const float* __restrict__ ms,
                                                                  const float* __restrict__ m2, const double* __restrict__ step,
                                                                  double tau, float tol, float stiff, int tol_zero, int max_steps,
                                                                  float* __restrict__ xo, float* __restrict__ yo,
                                                                  int32_t* __restrict__ steps, float* __restrict__ measure,
                                                                  int32_t* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int b = blockIdx.x;
    const int32_t* d = desc + GADAPT_MMPDE5_DESC * b;
    const double h = step[b];
    const Params p{(float)h, (float)(h / 6.0), tol, stiff, tol_zero, max_steps, tau};
#define STRIDED_RUN(DIM, K) mmpde5_run_strided<DIM, K>(d, x0, y0, ms, m2, p, xo, yo, steps + b, measure + b, status + b, lds)
    if (d[GADAPT_MMPDE5_D_DIM] != 2) {
        STRIDED_RUN(1, 1);
        return;
    }
    const int nodes = d[GADAPT_MMPDE5_D_N] * d[GADAPT_MMPDE5_D_N];
    switch ((nodes + strided_threads(nodes) - 1) / strided_threads(nodes)) {     // the same for every lane of the workgroup
        case 1: STRIDED_RUN(2, 1); break;
        case 2: STRIDED_RUN(2, 2); break;
        case 3: STRIDED_RUN(2, 3); break;
        case 4: STRIDED_RUN(2, 4); break;
        case 5: STRIDED_RUN(2, 5); break;
        case 6: STRIDED_RUN(2, 6); break;
        default: STRIDED_RUN(2, 7); break;               // the host admits no mesh beyond 81 x 81
    }
#undef STRIDED_RUN
}

}  // namespace

extern "C" int gadapt_mesh_abi_version(void) { return GADAPT_MESH_ABI; }
extern "C" const char* gadapt_mesh_last_error(void) { return g_err; }
extern "C" int gadapt_mmpde5_max_nodes(void) { return MAX_NODES; }
extern "C" int gadapt_mmpde5_max_steps(void) { return GADAPT_MMPDE5_MAX_STEPS; }

extern "C" int gadapt_mmpde5_threads(int nodes) {
    if (nodes < 3) return mesh_fail(GADAPT_MESH_E_BADARG, "gadapt_mmpde5_threads: a mesh has at least 3 nodes");
    if (nodes > MAX_NODES) return mesh_fail(GADAPT_MESH_E_SIZE, "gadapt_mmpde5_threads: more nodes than one workgroup holds");
    return mmpde5_threads(nodes);
}

extern "C" int64_t gadapt_mmpde5_lds_bytes(int nodes) {
    if (nodes < 3 || nodes > MAX_NODES) return mesh_fail(GADAPT_MESH_E_SIZE, "gadapt_mmpde5_lds_bytes: 3..1024 nodes");
    return 4 * mmpde5_lds_floats(nodes);
}

namespace {

// More than 64 KB of dynamic LDS needs the kernel's limit raised, once per device.
int allow_strided_lds() {
    static int done[64] = {0};                           // by device ordinal; a repeated call is harmless
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return -1;
    if (dev >= 0 && dev < 64 && __atomic_load_n(&done[dev], __ATOMIC_ACQUIRE)) return 0;
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(mmpde5_strided_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)(4 * mmpde5_lds_floats(STRIDED_MAX_NODES))) != hipSuccess)
        return -1;
    if (dev >= 0 && dev < 64) __atomic_store_n(&done[dev], 1, __ATOMIC_RELEASE);
    return 0;
}

int mmpde5_batch_route(const char* who, bool strided, int n_mesh, const int32_t* desc_host, const int32_t* desc, const float* x0,
                       const float* y0, const float* ms, const float* m2, const double* step, double tau, double tol,
                       int max_steps, float* x, float* y, int32_t* steps, float* measure, int32_t* status, void* stream) {
    char msg[240];
    if (n_mesh < 1 || !desc_host || !desc || !x0 || !ms || !m2 || !step || !x || !steps || !measure || !status) {
        snprintf(msg, sizeof msg, "%s: empty batch or null pointer", who);
        return mesh_fail(GADAPT_MESH_E_BADARG, msg);
    }
    if (!(tau > 0.0) || !(tol >= 0.0) || !isfinite(tau) || !isfinite(tol)) {
        snprintf(msg, sizeof msg, "%s: need tau > 0 and tol >= 0, both finite", who);
        return mesh_fail(GADAPT_MESH_E_BADARG, msg);
    }
    if (max_steps < 0 || max_steps > GADAPT_MMPDE5_MAX_STEPS) {
        snprintf(msg, sizeof msg, "%s: max_steps %d; 0..%d supported (the loop must end)", who, max_steps, GADAPT_MMPDE5_MAX_STEPS);
        return mesh_fail(GADAPT_MESH_E_SIZE, msg);
    }
    int threads = 64, most = 0;
    for (int b = 0; b < n_mesh; ++b) {
        const int32_t* d = desc_host + GADAPT_MMPDE5_DESC * b;
        const int dim = d[GADAPT_MMPDE5_D_DIM], N = d[GADAPT_MMPDE5_D_N];
        if ((dim != 1 && dim != 2) || N < 3 || d[GADAPT_MMPDE5_D_NODE_OFF] < 0 || d[GADAPT_MMPDE5_D_CELL_OFF] < 0) {
            snprintf(msg, sizeof msg, "%s: mesh %d: dimension %d, N %d, offsets %d / %d", who, b, dim, N, d[GADAPT_MMPDE5_D_NODE_OFF],
                     d[GADAPT_MMPDE5_D_CELL_OFF]);
            return mesh_fail(GADAPT_MESH_E_BADARG, msg);
        }
        if (strided ? (dim == 1 ? N > MAX_NODES : N > STRIDED_MAX_SIDE) : (N > MAX_NODES || (dim == 2 && N * N > MAX_NODES))) {
            if (strided)
                snprintf(msg, sizeof msg, "%s: mesh %d: N = %d in %d-D; 1-D N <= %d, 2-D N <= %d a side (one workgroup holds a mesh)",
                         who, b, N, dim, MAX_NODES, STRIDED_MAX_SIDE);
            else
                snprintf(msg, sizeof msg, "%s: mesh %d: N = %d in %d-D; at most %d nodes per mesh (1-D N <= 1024, 2-D N <= 32)", who,
                         b, N, dim, MAX_NODES);
            return mesh_fail(GADAPT_MESH_E_SIZE, msg);
        }
        if (dim == 2 && !(y0 && y)) {
            snprintf(msg, sizeof msg, "%s: a 2-D mesh needs y0 and y", who);
            return mesh_fail(GADAPT_MESH_E_BADARG, msg);
        }
        const int nodes = dim == 2 ? N * N : N;
        const int t = strided ? strided_threads(nodes) : mmpde5_threads(nodes);
        threads = t > threads ? t : threads;
        most = nodes > most ? nodes : most;
    }
    const float tol_f = (float)tol;
    const int tol_zero = tol_f == 0.0f;
    const float stiff = tol_zero ? INFINITY : (float)(1.0 / tol);
    const size_t lds = (size_t)(4 * mmpde5_lds_floats(most));
    if (strided) {
        if (lds > 64 * 1024 && allow_strided_lds() != 0) {
            (void)hipGetLastError();
            snprintf(msg, sizeof msg, "%s: %zu bytes of LDS refused (hipFuncSetAttribute)", who, lds);
            return mesh_fail(GADAPT_MESH_E_LAUNCH, msg);
        }
        mmpde5_strided_kernel<<<n_mesh, threads, lds, (hipStream_t)stream>>>(desc, x0, y0, ms, m2, step, tau, tol_f, stiff, tol_zero,
                                                                           max_steps, x, y, steps, measure, status);
    } else {
        mmpde5_kernel<<<n_mesh, threads, lds, (hipStream_t)stream>>>(desc, x0, y0, ms, m2, step, tau, tol_f, stiff, tol_zero, max_steps,
                                                                   x, y, steps, measure, status);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return mesh_fail(GADAPT_MESH_E_LAUNCH, hipGetErrorString(e));
    return GADAPT_MESH_OK;
}

}  // namespace

extern "C" int gadapt_mmpde5_strided_max_side(void) { return STRIDED_MAX_SIDE; }

extern "C" int64_t gadapt_mmpde5_strided_lds_bytes(int nodes) {
    if (nodes < 3 || nodes > STRIDED_MAX_NODES) return mesh_fail(GADAPT_MESH_E_SIZE, "gadapt_mmpde5_strided_lds_bytes: 3..6561 nodes");
    return 4 * mmpde5_lds_floats(nodes);
}

extern "C" int gadapt_mmpde5_batch(int n_mesh, const int32_t* desc_host, const int32_t* desc, const float* x0, const float* y0,
                                   const float* ms, const float* m2, const double* step, double tau, double tol, int max_steps,
                                   float* x, float* y, int32_t* steps, float* measure, int32_t* status, void* stream) {
    return mmpde5_batch_route("gadapt_mmpde5_batch", false, n_mesh, desc_host, desc, x0, y0, ms, m2, step, tau, tol, max_steps, x, y,
                              steps, measure, status, stream);
}

extern "C" int gadapt_mmpde5_batch_strided(int n_mesh, const int32_t* desc_host, const int32_t* desc, const float* x0,
                                           const float* y0, const float* ms, const float* m2, const double* step, double tau,
                                           double tol, int max_steps, float* x, float* y, int32_t* steps, float* measure,
                                           int32_t* status, void* stream) {
    return mmpde5_batch_route("gadapt_mmpde5_batch_strided", true, n_mesh, desc_host, desc, x0, y0, ms, m2, step, tau, tol, max_steps,
                              x, y, steps, measure, status, stream);
}
