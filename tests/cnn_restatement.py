"""The global CNN features (`src/feature_extractors.py:6-34`) written out tap by tap, in any dtype, in the order of operations of
the HIP kernels (`csrc/gadapt_cnn.inc`): the field divided by the batch maximum of its absolute value; then, per layer and output
channel, the bias, the input channels ascending and within each the taps ascending (row-major over the 3 or 3 x 3 window, zero outside
the image), one multiply-add each; SELU; after four layers the mean over pixels.  Differentiable torch code on the CPU: its fp64 run
is the yardstick of tests/test_gpu_cnn.py, its fp32 run the measure of how far fp32 arithmetic in this order sits from it."""
import torch
import torch.nn.functional as F

SELU_ALPHA = 1.6732632423543772848170429916717
SELU_SCALE = 1.0507009873554804934193349852946


def selu(z):
    return SELU_SCALE * torch.where(z > 0, z, SELU_ALPHA * torch.expm1(z))


def restatement(u, params, dim):
    """u [B, 1, n] / [B, 1, n0, n1], params (w0, b0, ..., w3, b3) -> (feat [B, out], [A_1, .., A_4] with A_l [B, C_l, n0 n1])."""
    B = u.shape[0]
    x = (u / u.abs().max()).reshape(B, 1, 1 if dim == 1 else u.shape[2], u.shape[-1])
    n0, n1 = x.shape[2], x.shape[3]
    acts = []
    for l in range(4):
        w, b = params[2 * l], params[2 * l + 1]
        w = w.reshape(w.shape[0], w.shape[1], 1 if dim == 1 else 3, 3)
        rows = w.shape[2]
        xp = F.pad(x, (1, 1, 1, 1) if rows == 3 else (1, 1, 0, 0))
        z = b.reshape(1, -1, 1, 1).expand(B, -1, n0, n1)
        for ci in range(w.shape[1]):
            for ky in range(rows):
                for kx in range(3):
                    z = z + w[:, ci, ky, kx].reshape(1, -1, 1, 1) * xp[:, ci:ci + 1, ky:ky + n0, kx:kx + n1]
        x = selu(z)
        acts.append(x.reshape(B, x.shape[1], n0 * n1))
    return x.sum(dim=(2, 3)) / (n0 * n1), acts
