"""Global (per-mesh) CNN features of the PDE fields: `src/feature_extractors.py:6-34` and their use in
`GNN.forward` (`src/GNN.py:240-268`).

A caller either side of the message-passing path, not part of it: four 3x3 convolutions with
SELU on the n x n grid of a field, global average pool -> `global_feat_dim` numbers per mesh, repeated for every node of
that mesh and appended to the node features.  The parameters live in torch `nn.Conv1d/2d` modules with the reference's
names, so `state_dict`s interchange; gradients reach them through the encoder input (`functional.grand_euler_block` returns
d/dx0 when x0 requires grad).

Two routes compute them (`GlobalFeatureExtractorCNN(kernel=...)`, `opt['glob_feat_kernel']`): 'torch', the default - the modules
themselves (MIOpen on ROCm) - and 'hip', `global_cnn`: one launch forward and one backward with one workgroup per mesh
(`csrc/gadapt_cnn.inc`), for images whose LDS copies fit 64 KB (`hip_limit`).  'auto' takes 'hip' where it fits.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _native
from ._native import NativeError

KERNELS = ('torch', 'hip', 'auto')
LDS_BUDGET = 65536          # bytes of LDS a workgroup gets without asking for more: csrc/gadapt_cnn_plan.h


def hip_limit(dim: int, n0: int, n1: int, mid: int, out: int, training: bool = True) -> Optional[str]:
    """None if `global_cnn` takes this image, else the sentence that names the limit.  The forward keeps two LDS images of
    (n0 + 2)(n1 + 2) max(mid, out) floats, the backward three, both beside n0 n1 pixel offsets; a call that records for a backward
    must fit the backward."""
    lib = _native.lib()
    need = (lib.gadapt_cnn_backward_lds_bytes if training else lib.gadapt_cnn_forward_lds_bytes)(dim, n0, n1, mid, out)
    if need < 0:
        return f"global_cnn: dim {dim}, image {n0} x {n1}, channels {mid} / {out}: dim 1 (n0 = 1) or 2, sizes of 1 or more"
    if need > LDS_BUDGET:
        return (f"global_cnn: the {'backward' if training else 'forward'} of a {n0} x {n1} image with {mid} / {out} channels needs "
                f"{need} bytes of LDS ({3 if training else 2} images of (n0 + 2)(n1 + 2) max(mid, out) floats and n0 n1 offsets), above the {LDS_BUDGET}-byte budget")
    return None


def _image_shape(u: torch.Tensor, dim: int):
    if u.dim() != dim + 2 or u.shape[1] != 1:
        raise ValueError(f"global_cnn: the field is [B, 1, n] at dim 1 and [B, 1, n0, n1] at dim 2, got {tuple(u.shape)} at dim {dim}")
    return (1, int(u.shape[2])) if dim == 1 else (int(u.shape[2]), int(u.shape[3]))


class _GlobalCNN(torch.autograd.Function):
    """The two launches of include/gadapt_hip.h (gadapt_cnn_forward / gadapt_cnn_backward).  The field is data: no gradient."""

    @staticmethod
    def forward(ctx, u, dim, *params):
        lib = _native.lib()
        B, (n0, n1) = int(u.shape[0]), _image_shape(u, dim)
        mid, out = int(params[0].shape[0]), int(params[6].shape[0])
        umax = torch.amax(torch.abs(u))                      # stays on the device: nothing here reads it on the host
        feat = torch.empty(B, out, device=u.device, dtype=torch.float32)
        train = any(ctx.needs_input_grad[2:])                # (grad mode is off in here; this is what the caller's mode decided)
        acts = torch.empty(lib.gadapt_cnn_workspace_floats(B, dim, n0, n1, mid, out), device=u.device, dtype=torch.float32) if train else None
        _native.check(lib.gadapt_cnn_forward(_native.ptr(u), _native.ptr(umax), B, dim, n0, n1, mid, out, *[_native.ptr(p) for p in params],
                                             _native.ptr(feat), _native.ptr(acts), _native.current_stream(u.device)), 'gadapt_cnn_forward')
        if train:
            ctx.save_for_backward(u, umax, acts, *params)
            ctx.sizes = (B, dim, n0, n1, mid, out)
        return feat

    @staticmethod
    def backward(ctx, d_feat):
        lib = _native.lib()
        u, umax, acts, *params = ctx.saved_tensors
        B, dim, n0, n1, mid, out = ctx.sizes
        n_params = lib.gadapt_cnn_param_floats(dim, mid, out)
        d_feat = d_feat.contiguous().float()
        d_params = torch.empty(n_params, device=u.device, dtype=torch.float32)
        partials = torch.empty(B, n_params, device=u.device, dtype=torch.float32) if B > 1 else None
        _native.check(lib.gadapt_cnn_backward(_native.ptr(d_feat), _native.ptr(acts), _native.ptr(u), _native.ptr(umax), B, dim, n0, n1, mid, out,
                                              *[_native.ptr(p) for p in params], _native.ptr(partials), _native.ptr(d_params),
                                              _native.current_stream(u.device)), 'gadapt_cnn_backward')
        grads = [g.view_as(p) for g, p in zip(torch.split(d_params, [p.numel() for p in params]), params)]
        return (None, None, *grads)


def global_cnn(u: torch.Tensor, params: Sequence[torch.Tensor], dim: int) -> torch.Tensor:
    """[B, 1, n] / [B, 1, n0, n1] field -> [B, out] features of the four-layer CNN on the HIP kernels.  `params` = (w0, b0, ..., w3,
    b3) as `nn.Conv1d` / `nn.Conv2d` hold them ([out, in, 3] / [out, in, 3, 3]; channels 1 -> mid -> mid -> mid -> out)."""
    params = tuple(params)
    if dim not in (1, 2) or len(params) != 8:
        raise ValueError("global_cnn: dim 1 or 2 and the eight tensors of four convolutions (w0, b0, ..., w3, b3)")
    n0, n1 = _image_shape(u, dim)
    mid, out = int(params[0].shape[0]), int(params[6].shape[0])
    taps = (3,) * dim
    want = [(mid, 1), (mid, mid), (mid, mid), (out, mid)]
    for k, (co, ci) in enumerate(want):
        if tuple(params[2 * k].shape) != (co, ci) + taps or tuple(params[2 * k + 1].shape) != (co,):
            raise ValueError(f"global_cnn: convolution {k} is not {ci} -> {co} channels with {'x'.join(map(str, taps))} taps: four layers "
                             "1 -> mid -> mid -> mid -> out only")
    if u.requires_grad:
        raise ValueError("global_cnn: the field is data, no gradient is computed for it")
    if not u.is_cuda or u.dtype != torch.float32 or any(p.dtype != torch.float32 or p.device != u.device for p in params):
        raise NativeError("global_cnn: fp32 tensors on one GPU (there is no CPU fallback: kernel='torch' runs anywhere)")
    train = torch.is_grad_enabled() and any(p.requires_grad for p in params)
    why = hip_limit(dim, n0, n1, mid, out, training=train)
    if why:
        raise NativeError(why)
    return _GlobalCNN.apply(u.contiguous(), dim, *[p.contiguous() for p in params])


class GlobalFeatureExtractorCNN(nn.Module):
    """`convs.{k}.{weight,bias}`: in -> mid -> ... -> mid -> out, all 3x3 (or 3), stride 1, padding 1.

    kernel: 'torch' (the default) runs the modules; 'hip' runs `global_cnn` and raises `NativeError` naming the limit for an image it
    does not take; 'auto' runs `global_cnn` where it fits and the modules otherwise.  The parameters are the same either way."""

    def __init__(self, in_channels: int, mid_channels: int, out_channels: int, dim: int = 2, num_layers: int = 4, kernel: str = 'torch'):
        super().__init__()
        if kernel not in KERNELS:
            raise ValueError(f"GlobalFeatureExtractorCNN: kernel must be one of {KERNELS}, got {kernel!r}")
        if kernel == 'hip' and (in_channels != 1 or num_layers != 4):
            raise ValueError("GlobalFeatureExtractorCNN: kernel='hip' is built for one input channel and four layers")
        conv = {1: nn.Conv1d, 2: nn.Conv2d}[dim]
        widths = [in_channels] + [mid_channels] * (num_layers - 1) + [out_channels]
        self.convs = nn.ModuleList([conv(a, b, kernel_size=3, stride=1, padding=1) for a, b in zip(widths[:-1], widths[1:])])
        self.global_avg_pool = {1: nn.AdaptiveAvgPool1d(1), 2: nn.AdaptiveAvgPool2d((1, 1))}[dim]
        self.dim, self.kernel = dim, kernel
        self._hip_shape = in_channels == 1 and num_layers == 4

    def _takes_hip(self, u: torch.Tensor) -> bool:
        if self.kernel == 'hip':
            return True
        if self.kernel != 'auto' or not self._hip_shape or not u.is_cuda or u.dtype != torch.float32 or u.requires_grad:
            return False
        n0, n1 = _image_shape(u, self.dim)
        train = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        return hip_limit(self.dim, n0, n1, self.convs[0].out_channels, self.convs[3].out_channels, training=train) is None

    def forward(self, u: torch.Tensor) -> torch.Tensor:
        if self.kernel != 'torch' and self._takes_hip(u):
            return global_cnn(u, [t for conv in self.convs for t in (conv.weight, conv.bias)], self.dim)
        u = u / torch.max(torch.abs(u))                     # one scale for the whole batch (feature_extractors.py:29)
        for conv in self.convs:
            u = F.selu(conv(u))
        return self.global_avg_pool(u).flatten(1)           # [B, out_channels]


def field_to_grid(field: torch.Tensor, mapping: Optional[torch.Tensor], mesh_dims: Sequence[int], batch_size: int,
                  dim: int) -> torch.Tensor:
    """Node-ordered field [B*n^d] -> CNN grid [B, n] / [B, n, n] (`src/utils_data.py:125-141`): per mesh, nodes are
    picked in `mapping` order, laid out row-major, then transposed and flipped along the first grid axis."""
    per_mesh = field.reshape(batch_size, -1)
    if dim == 1:
        return per_mesh
    if mapping is not None:
        per_mesh = per_mesh.index_select(1, mapping.to(per_mesh.device))
    return per_mesh.reshape(batch_size, mesh_dims[0], mesh_dims[1]).transpose(1, 2).flip(1)


class _ExpandRows(torch.autograd.Function):
    """`per_mesh[batch]` whose backward sums each mesh's node rows in a fixed order.  `index_select`'s own backward is an
    `index_add_` on floating-point atomics: the order of a mesh's rows, and with it the last bits of the gradient every extractor
    parameter gets, changes from run to run.  The meshes of a batch have one size here (`field_to_grid` reshapes by it), so the
    sum over a mesh's nodes is the reduction of a [B, n, k] view."""

    @staticmethod
    def forward(ctx, per_mesh, batch):
        ctx.n_meshes = per_mesh.shape[0]
        return per_mesh.index_select(0, batch)

    @staticmethod
    def backward(ctx, grad):
        return grad.reshape(ctx.n_meshes, -1, grad.shape[1]).sum(1), None


def expand_to_nodes(per_mesh: torch.Tensor, batch: torch.Tensor, fixed_order: bool = False) -> torch.Tensor:
    """[B, k] -> [N, k]: every node gets its mesh's row (`repeat_interleave(bincount(batch))`, GNN.py:252-253).  `batch` is the
    sorted mesh index of every node, so the repeat IS the row gather `per_mesh[batch]` - which, unlike `bincount` +
    `repeat_interleave` (data-dependent output size: a host synchronisation), can sit inside a captured hipGraph.
    fixed_order: the same rows with a backward that has no atomics (`_ExpandRows`; equal-sized meshes) - what the 'hip' route of the
    extractors asks for, so that its fixed-order gradients start from fixed-order seeds."""
    if fixed_order and per_mesh.requires_grad and batch.shape[0] % per_mesh.shape[0] == 0:
        return _ExpandRows.apply(per_mesh, batch)
    return per_mesh.index_select(0, batch)
