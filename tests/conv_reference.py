"""Plain-torch CPU reference of the convolution operators of `sast_amd.functional` (conv_bn_silu, conv_bn_silu2 as two units,
downsample_ln, dwconv, upsample_cat, cat2).

Every function computes in the dtype of the tensors it is given: float64 for the reference the HIP kernels are compared with
(tests/test_conv_operators.py), float32 for the error of that very expression in fp32 (tests/golden/make_operator_bounds.py).  Tensors are
NHWC like the library's ("image layout" rows [B*H*W, C]); weights have their logical nn.Conv2d shape [Cout, Cin / groups, k, k].
Gradients come from autograd through these expressions.  Nothing here knows about the library or the oracle; tests/test_conv_reference.py
pins it against torch.nn modules.
"""
import torch
import torch.nn.functional as F


def nchw(x):
    return x.permute(0, 3, 1, 2)


def nhwc(x):
    return x.permute(0, 2, 3, 1)


def conv_out_size(n, k, stride, pad):
    return (n + 2 * pad - k) // stride + 1


def conv_bn_silu(x, w, bn_w, bn_b, run_mean, run_var, ksize, stride, mode, momentum=0.1, eps=1e-5):
    """Conv2d(k, stride, padding (k-1)//2, no bias) -> BatchNorm2d -> SiLU.
    x: NHWC tensor, or a pair (xa, xb) standing for their channel concat.  w [Cout, Cin, k, k] dense or [C, 1, k, k] depth-wise
    (groups = C).  mode: "train" (batch statistics; the running statistics move), "eval" (running statistics, differentiable),
    "infer" (the same without autograd).  -> (y NHWC, running_mean after the call, running_var after the call)"""
    if mode == "infer":
        with torch.no_grad():
            return conv_bn_silu(x, w, bn_w, bn_b, run_mean, run_var, ksize, stride, "eval", momentum, eps)
    if isinstance(x, (tuple, list)):
        x = torch.cat(tuple(x), dim=-1)
    cin = x.shape[-1]
    groups = 1 if w.shape[1] == cin else cin
    z = F.conv2d(nchw(x), w, None, stride, (ksize - 1) // 2, 1, groups)
    if mode == "train":
        n = z.numel() // z.shape[1]
        mean = z.mean(dim=(0, 2, 3))
        var = ((z - mean.view(1, -1, 1, 1)) ** 2).mean(dim=(0, 2, 3))          # biased: what normalises
        new_mean = (1 - momentum) * run_mean + momentum * mean.detach()
        new_var = (1 - momentum) * run_var + momentum * var.detach() * (n / (n - 1))      # unbiased: what is remembered
    else:
        assert mode == "eval", mode
        mean, var, new_mean, new_var = run_mean, run_var, run_mean, run_var
    zh = (z - mean.view(1, -1, 1, 1)) / torch.sqrt(var.view(1, -1, 1, 1) + eps) * bn_w.view(1, -1, 1, 1) + bn_b.view(1, -1, 1, 1)
    return nhwc(zh * torch.sigmoid(zh)), new_mean, new_var


def downsample_ln(x, w, ln_w, ln_b, pe, factor):
    """the factor-f downsampling conv (no bias) + LayerNorm(eps 1e-5, affine) (+ position table).  Kernel 2f-1: replicate padding f-1
    (overlap); kernel f: no padding.  x NHWC (uint8 is widened to w's dtype), pe [Ho*Wo, Cout] or None: added AFTER the norm, the same
    table for every sample."""
    k = w.shape[-1]
    xc = nchw(x.to(w.dtype))
    if k == 2 * factor - 1:
        xc = F.pad(xc, (factor - 1,) * 4, mode="replicate")
    else:
        assert k == factor, (k, factor)
    z = nhwc(F.conv2d(xc, w, None, factor))
    y = F.layer_norm(z, (z.shape[-1],), ln_w, ln_b, 1e-5)
    if pe is not None:
        y = y + pe.view(1, z.shape[1], z.shape[2], z.shape[3])
    return y


def dwconv(x, w, b, c0=0):
    """depth-wise k x k conv, zero padding k // 2, stride 1, of the C channels of x with the channels [c0, c0 + C) of the parameters
    w [Cw, 1, k, k], b [Cw] or None"""
    C, k = x.shape[-1], w.shape[-1]
    return nhwc(F.conv2d(nchw(x), w[c0:c0 + C], None if b is None else b[c0:c0 + C], 1, k // 2, 1, C))


def upsample_cat(a, b):
    """cat(nearest x2 of a, b) along channels"""
    return torch.cat((a.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2), b), dim=-1)


def cat2(a, b):
    return torch.cat((a, b), dim=-1)
