// gadapt_tu_cnn.hip - the global CNN features of a field (features.GlobalFeatureExtractorCNN, kernel='hip'): one launch forward, one
// launch backward plus a fixed-order sum over meshes, one workgroup per mesh (gadapt_cnn.inc; sizes and limits: gadapt_cnn_plan.h).
// One translation unit of libgadapt_hip.so (see gadapt_internal.h).
#include "gadapt_internal.h"
#include "gadapt_cnn_plan.h"
#include "gadapt_cnn.inc"

extern "C" int64_t gadapt_cnn_forward_lds_bytes(int dim, int n0, int n1, int mid, int out) {
    return cnn_plan::sizes_ok(dim, n0, n1, mid, out) ? cnn_plan::forward_lds_bytes(n0, n1, mid, out) : -1;
}
extern "C" int64_t gadapt_cnn_backward_lds_bytes(int dim, int n0, int n1, int mid, int out) {
    return cnn_plan::sizes_ok(dim, n0, n1, mid, out) ? cnn_plan::backward_lds_bytes(n0, n1, mid, out) : -1;
}
extern "C" int64_t gadapt_cnn_workspace_floats(int n_meshes, int dim, int n0, int n1, int mid, int out) {
    return n_meshes >= 1 && cnn_plan::sizes_ok(dim, n0, n1, mid, out) ? cnn_plan::workspace_floats(n_meshes, n0, n1, mid, out) : -1;
}
extern "C" int gadapt_cnn_param_floats(int dim, int mid, int out) {
    if (!cnn_plan::sizes_ok(dim, 1, 1, mid, out)) return -1;
    const int64_t n = cnn_plan::param_floats(dim, mid, out);
    return n < ((int64_t)1 << 31) ? (int)n : -1;
}

static bool any_null(const cnn::Params& p) {
    for (int l = 0; l < cnn::L; ++l) if (!p.w[l] || !p.b[l]) return true;
    return false;
}

extern "C" int gadapt_cnn_forward(const float* u, const float* umax, int n_meshes, int dim, int n0, int n1, int mid, int out,
                                  const float* w0, const float* b0, const float* w1, const float* b1, const float* w2, const float* b2,
                                  const float* w3, const float* b3, float* feat, float* acts, void* stream) {
    const cnn::Params p{{w0, w1, w2, w3}, {b0, b1, b2, b3}};
    if (!u || !umax || !feat || any_null(p)) return fail(GADAPT_E_BADARG, "cnn_forward: null pointer");
    char why[256];
    if (cnn_plan::refuse("cnn_forward", n_meshes, dim, n0, n1, mid, out, 2, why, sizeof(why))) return fail(GADAPT_E_BADARG, why);
    const cnn::FwdArgs a{u, umax, p, feat, acts, n_meshes, n0, n1, mid, out};
    const int lds = (int)cnn_plan::forward_lds_bytes(n0, n1, mid, out), nt = cnn_plan::forward_threads(n0, n1, mid, out);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (dim == 1) hipLaunchKernelGGL(cnn::cnn_forward_kernel<1>, dim3(n_meshes), dim3(nt), lds, st, a);
    else hipLaunchKernelGGL(cnn::cnn_forward_kernel<2>, dim3(n_meshes), dim3(nt), lds, st, a);
    return check_launch("cnn_forward_kernel");
}

extern "C" int gadapt_cnn_backward(const float* d_feat, const float* acts, const float* u, const float* umax, int n_meshes, int dim, int n0, int n1,
                                   int mid, int out, const float* w0, const float* b0, const float* w1, const float* b1, const float* w2,
                                   const float* b2, const float* w3, const float* b3, float* partials, float* d_params, void* stream) {
    const cnn::Params p{{w0, w1, w2, w3}, {b0, b1, b2, b3}};
    if (!d_feat || !acts || !u || !umax || !d_params || (!partials && n_meshes > 1) || any_null(p)) return fail(GADAPT_E_BADARG, "cnn_backward: null pointer");
    char why[256];
    if (cnn_plan::refuse("cnn_backward", n_meshes, dim, n0, n1, mid, out, 3, why, sizeof(why))) return fail(GADAPT_E_BADARG, why);
    const int64_t n_params = cnn_plan::param_floats(dim, mid, out);
    if (n_params * n_meshes >= ((int64_t)1 << 31)) return fail(GADAPT_E_BADARG, "cnn_backward: 2^31 gradient partials or more");
    // one mesh: its partials ARE the gradient
    cnn::BwdArgs a{u, umax, acts, d_feat, p, n_meshes == 1 ? d_params : partials, n_meshes, n0, n1, mid, out, {0, 0, 0, 0}, (int)n_params};
    for (int l = 0; l < cnn::L; ++l) a.poff[l] = (int)cnn_plan::param_offset(l, dim, mid, out);
    const int lds = (int)cnn_plan::backward_lds_bytes(n0, n1, mid, out), nt = cnn_plan::backward_threads(dim, n0, n1, mid, out);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (dim == 1) hipLaunchKernelGGL(cnn::cnn_backward_kernel<1>, dim3(n_meshes), dim3(nt), lds, st, a);
    else hipLaunchKernelGGL(cnn::cnn_backward_kernel<2>, dim3(n_meshes), dim3(nt), lds, st, a);
    if (n_meshes > 1)
        hipLaunchKernelGGL(cnn::cnn_reduce_kernel, dim3((unsigned)((n_params + 255) / 256)), dim3(256), 0, st, partials, d_params, n_meshes, (int)n_params);
    return check_launch("cnn_backward_kernel");
}
