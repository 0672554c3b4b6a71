// gadapt_cnn_plan.h - sizes and limits of the global CNN features (gadapt_tu_cnn.hip, gadapt_cnn.inc): plain host C++, no HIP, so
// the C-ABI, the kernels' host side and tools/cnn_plan_sweep.cpp (sanitizer builds) share ONE definition.
//
// The network: channels 1 -> mid -> mid -> mid -> out, four layers, 3 (dim 1) or 3 x 3 (dim 2) taps, stride 1, zero padding 1, SELU after
// every layer, average pool.  One image shape per call, [n0][n1], 1-D is n0 = 1.  An LDS image is channel-major with a zero halo:
// max(mid, out) planes of (n0 + 2)(n1 + 2) floats.  The forward holds two (ping-pong), the backward three (A_{l-1}, dZ_l, dA_{l-1}); both
// also hold one table of n0 n1 ints, pixel -> offset of that pixel in a plane, so that no loop over pixels divides by n1.  Both stay
// within the 64 KB a launch gets without the dynamic-LDS attribute.  (The table is what decides 24 x 24 at 8 channels: its three
// images alone are 64 896 bytes.)
#ifndef GADAPT_CNN_PLAN_H
#define GADAPT_CNN_PLAN_H
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#define GADAPT_CNN_LDS_BUDGET 65536     /* bytes: the default dynamic-LDS limit of a launch */
#define GADAPT_CNN_LAYERS 4
#define GADAPT_CNN_MAX_WAVES 16         /* 1024-thread workgroups at most */
#define GADAPT_CNN_MAX_SIDE 4096        /* n0, n1: keeps every size below in 64 bits with room (the LDS budget is the real limit) */
#define GADAPT_CNN_MAX_CHANNELS 4096

namespace cnn_plan {

inline bool sizes_ok(int dim, int n0, int n1, int mid, int out) {
    return (dim == 1 || dim == 2) && n0 >= 1 && n1 >= 1 && (dim == 2 || n0 == 1) && n0 <= GADAPT_CNN_MAX_SIDE && n1 <= GADAPT_CNN_MAX_SIDE
        && mid >= 1 && out >= 1 && mid <= GADAPT_CNN_MAX_CHANNELS && out <= GADAPT_CNN_MAX_CHANNELS;
}
inline int taps(int dim) { return dim == 1 ? 3 : 9; }
inline int64_t pixels(int n0, int n1) { return (int64_t)n0 * n1; }
inline int64_t plane_floats(int n0, int n1) { return (int64_t)(n0 + 2) * (n1 + 2); }
inline int64_t image_floats(int n0, int n1, int mid, int out) { return plane_floats(n0, n1) * (mid > out ? mid : out); }
// channels in / out of layer l (0..3)
inline int c_in(int l, int mid) { return l == 0 ? 1 : mid; }
inline int c_out(int l, int mid, int out) { return l == GADAPT_CNN_LAYERS - 1 ? out : mid; }
// packed parameters: w0, b0, w1, b1, w2, b2, w3, b3; w_l is [c_out][c_in][taps] (Conv1d [out, in, 3], Conv2d [out, in, 3, 3])
inline int64_t weight_floats(int l, int dim, int mid, int out) { return (int64_t)c_out(l, mid, out) * c_in(l, mid) * taps(dim); }
inline int64_t param_offset(int l, int dim, int mid, int out) {                  // of w_l; b_l follows it
    int64_t o = 0;
    for (int k = 0; k < l; ++k) o += weight_floats(k, dim, mid, out) + c_out(k, mid, out);
    return o;
}
inline int64_t param_floats(int dim, int mid, int out) { return param_offset(GADAPT_CNN_LAYERS, dim, mid, out); }
// saved activations [4][B, C_l, n0 n1]: layer l starts at acts_offset(l)
inline int64_t acts_offset(int l, int64_t n_meshes, int n0, int n1, int mid, int out) {
    int64_t o = 0;
    for (int k = 0; k < l; ++k) o += n_meshes * c_out(k, mid, out) * pixels(n0, n1);
    return o;
}
inline int64_t workspace_floats(int64_t n_meshes, int n0, int n1, int mid, int out) { return acts_offset(GADAPT_CNN_LAYERS, n_meshes, n0, n1, mid, out); }

inline int64_t forward_lds_bytes(int n0, int n1, int mid, int out) { return 4 * (2 * image_floats(n0, n1, mid, out) + pixels(n0, n1)); }
inline int64_t backward_lds_bytes(int n0, int n1, int mid, int out) { return 4 * (3 * image_floats(n0, n1, mid, out) + pixels(n0, n1)); }

// What a call is refused for before anything is launched (NULL: nothing); the text goes to gadapt_last_error().  images: 2 (forward)
// or 3 (backward).
inline const char* refuse(const char* who, int n_meshes, int dim, int n0, int n1, int mid, int out, int images, char* buf, size_t cap) {
    if (n_meshes < 1) { snprintf(buf, cap, "%s: n_meshes < 1", who); return buf; }
    if (dim != 1 && dim != 2) { snprintf(buf, cap, "%s: dim must be 1 or 2", who); return buf; }
    if (!sizes_ok(dim, n0, n1, mid, out)) {
        snprintf(buf, cap, "%s: 1 <= n0, n1 <= %d (n0 = 1 when dim = 1), 1 <= mid, out <= %d", who, GADAPT_CNN_MAX_SIDE, GADAPT_CNN_MAX_CHANNELS);
        return buf;
    }
    const int64_t need = images == 2 ? forward_lds_bytes(n0, n1, mid, out) : backward_lds_bytes(n0, n1, mid, out);
    if (need > GADAPT_CNN_LDS_BUDGET) {
        snprintf(buf, cap, "%s: %d LDS images of (n0 + 2)(n1 + 2) max(mid, out) floats and n0 n1 offsets = %lld bytes, above the %d-byte LDS budget of a workgroup "
                 "(n0 = %d, n1 = %d, mid = %d, out = %d)", who, images, (long long)need, GADAPT_CNN_LDS_BUDGET, n0, n1, mid, out);
        return buf;
    }
    if ((int64_t)n_meshes * (3 * (int64_t)mid + out) * pixels(n0, n1) >= ((int64_t)1 << 31)) { snprintf(buf, cap, "%s: workspace of 2^31 floats or more", who); return buf; }
    return nullptr;
}

// Workgroup size: a wave takes a unit of 64 pixels x 4 output channels at a time; as many waves as the widest layer has units,
// 4 .. 16.  The backward's weight-gradient lanes (one per (co, ci, tap) entry) want a full workgroup as soon as there are that many.
inline int threads_for(int64_t units) {
    int64_t w = units < 4 ? 4 : (units > GADAPT_CNN_MAX_WAVES ? GADAPT_CNN_MAX_WAVES : units);
    return (int)(64 * ((w + 3) / 4 * 4));
}
inline int64_t conv_units(int n0, int n1, int mid, int out) {
    const int c = mid > out ? mid : out;
    return ((pixels(n0, n1) + 63) / 64) * ((c + 3) / 4);
}
inline int forward_threads(int n0, int n1, int mid, int out) { return threads_for(conv_units(n0, n1, mid, out)); }
inline int backward_threads(int dim, int n0, int n1, int mid, int out) {
    const int64_t entries = ((int64_t)mid * mid * taps(dim) + mid + 63) / 64, units = conv_units(n0, n1, mid, out);
    return threads_for(entries > units ? entries : units);
}

}  // namespace cnn_plan
#endif  // GADAPT_CNN_PLAN_H
