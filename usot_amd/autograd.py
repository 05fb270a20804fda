"""torch.autograd bindings of the native depthwise cross-correlation (reference lib/models/connect.py:86-102,147-157), of
the fp32 convolution (every nn.Conv2d of connect.py), of BatchNorm2d with its ReLU (every nn.BatchNorm2d of connect.py), of
Conf_Fusion's clamp - exp - normalise - weighted sum (connect.py:129-142) and of the box epilogue exp(adjust * p + bias)
(connect.py:236-237).

Forward values are `usot_amd.hip.xcorr_depthwise`'s, `usot_amd.hip.conv2d`'s, `usot_amd.hip.batch_norm_forward`'s,
`usot_amd.hip.conf_fusion_forward`'s and `usot_amd.hip.box_exp_forward`'s, bit for bit; the gradients come from the kernels of
csrc/xcorr_grad.hip, csrc/conv_grad.hip, csrc/batchnorm.hip and csrc/head_grad.hip.  First-order gradients only, fp32 only,
device tensors only (no CPU implementation: CPU tensors raise `hip.HipError`).
"""
import torch
from torch.autograd.function import once_differentiable

from . import hip


class XCorrDepthwiseFunction(torch.autograd.Function):
    """out[b][c] = x[b][c] (*) kernel[b][c] (valid cross-correlation, one template per plane)."""

    @staticmethod
    def forward(ctx, x, kernel):
        ctx.save_for_backward(x, kernel)
        return hip.xcorr_depthwise(x, kernel)

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        x, kernel = ctx.saved_tensors
        dx = dk = None
        if ctx.needs_input_grad[0]:
            dx = hip.xcorr_depthwise_backward_x(dout, kernel, x.shape)
        if ctx.needs_input_grad[1]:
            dk = hip.xcorr_depthwise_backward_k(dout, x, kernel.shape)
        return dx, dk


def _wants_grad(*tensors):
    return torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in tensors)


def xcorr_depthwise(x, kernel):
    """Differentiable drop-in for the reference's `xcorr_depthwise` on NCHW device tensors."""
    if _wants_grad(x, kernel):
        hip._dev(x), hip._dev(kernel)
        return XCorrDepthwiseFunction.apply(x, kernel)
    return hip.xcorr_depthwise(x, kernel)


def _groupdw_forward(zs, xs, weight):
    w = torch.softmax(weight.detach(), 0)
    wl = w.tolist()                      # host copies: the gradient kernels take the branch weight as a scalar argument
    out = hip.xcorr_depthwise(xs[0], zs[0]).mul_(wl[0])
    for i in (1, 2):
        out.add_(hip.xcorr_depthwise(xs[i], zs[i]).mul_(wl[i]))
    return out, w, wl


class GroupDWFunction(torch.autograd.Function):
    """sum_i softmax(weight)[i] * xcorr(x_i, z_i).  The branch weights reach the gradient kernels as `scale`, and the
    gradient of `weight` is rebuilt from s_i = <dout, xcorr(x_i, z_i)> = <dk_i at scale 1, z_i>: no correlation map
    is saved."""

    @staticmethod
    def forward(ctx, weight, z0, z1, z2, x0, x1, x2):
        zs, xs = (z0, z1, z2), (x0, x1, x2)
        out, w, ctx.wl = _groupdw_forward(zs, xs, weight)
        ctx.save_for_backward(w, *zs, *xs)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        w, zs, xs = ctx.saved_tensors[0], ctx.saved_tensors[1:4], ctx.saved_tensors[4:7]
        need_w = ctx.needs_input_grad[0]
        wl = ctx.wl
        dz, dx, s = [None] * 3, [None] * 3, []
        for i in range(3):
            if ctx.needs_input_grad[4 + i]:
                dx[i] = hip.xcorr_depthwise_backward_x(dout, zs[i], xs[i].shape, wl[i])
            if need_w:
                dk1 = hip.xcorr_depthwise_backward_k(dout, xs[i], zs[i].shape)
                s.append((dk1 * zs[i]).sum(dtype=torch.float64))
                if ctx.needs_input_grad[1 + i]:
                    dz[i] = dk1.mul_(w[i])
            elif ctx.needs_input_grad[1 + i]:
                dz[i] = hip.xcorr_depthwise_backward_k(dout, xs[i], zs[i].shape, wl[i])
        dweight = None
        if need_w:
            s = torch.stack(s)                                       # float64: three numbers
            w64 = w.double()
            dweight = (w64 * (s - (w64 * s).sum())).to(w.dtype)      # softmax Jacobian, (diag(w) - w w^T) s
        return (dweight, *dz, *dx)


def groupdw(z, x, weight):
    """The reference's `GroupDW.forward`: `z`, `x` triples of NCHW device tensors (templates / search maps of the
    5x5, 3x5 and 5x3 branches), `weight` the three branch logits."""
    zs, xs = tuple(z), tuple(x)
    if len(zs) != 3 or len(xs) != 3:
        raise ValueError('groupdw: three templates and three search maps expected')
    for t in zs + xs:
        hip._dev(t)
    hip._dev(weight)
    if _wants_grad(weight, *zs, *xs):
        return GroupDWFunction.apply(weight, *zs, *xs)
    return _groupdw_forward(zs, xs, weight)[0]


def _pair(v):
    return (int(v), int(v)) if isinstance(v, int) else (int(v[0]), int(v[1]))


def _pack_oihw(weight):
    """OIHW -> the packed bank [Cout][KH*KW*Cin] of usot_conv_desc (k = (kh*KW + kw)*Cin + ci)"""
    return weight.permute(0, 2, 3, 1).reshape(weight.shape[0], -1).contiguous()


def _conv2d_forward(x, weight, bias, stride, pad, dil, relu):
    """(x NHWC, packed bank, y NHWC): `hip.conv2d` on the heuristic tile"""
    xh = hip.to_nhwc(x).contiguous()
    wp = _pack_oihw(weight)
    y = hip.conv2d(xh, wp, bias, KH=weight.shape[2], KW=weight.shape[3], stride=stride, pad=pad, dil=dil,
                   act=hip.ACT_RELU if relu else hip.ACT_NONE)
    return xh, wp, y


class Conv2dFunction(torch.autograd.Function):
    """y = [relu](conv2d(x, weight) + bias) on NCHW tensors and an OIHW weight; the kernels work on NHWC maps and the packed
    bank, which is what backward keeps."""

    @staticmethod
    def forward(ctx, x, weight, bias, stride, pad, dil, relu):
        xh, wp, y = _conv2d_forward(x.detach(), weight.detach(), None if bias is None else bias.detach(), stride, pad, dil, relu)
        ctx.geo = (tuple(weight.shape), stride, pad, dil, relu)
        ctx.save_for_backward(xh, wp, y if relu else None)
        return y.permute(0, 3, 1, 2)

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        xh, wp, y = ctx.saved_tensors
        (cout, cin, kh, kw), stride, pad, dil, relu = ctx.geo
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        dy = hip.to_nhwc(dout)
        dy = dy * (y > 0) if relu else dy.contiguous()
        dx = dw = db = None
        if need_x:
            dx = hip.conv2d_backward_x(dy, wp, xh.shape, KH=kh, KW=kw, stride=stride, pad=pad, dil=dil).permute(0, 3, 1, 2)
        if need_w or need_b:
            dwp, db = hip.conv2d_backward_w(xh, dy, KH=kh, KW=kw, stride=stride, pad=pad, dil=dil, bias=need_b)
            if need_w:
                dw = dwp.view(cout, kh, kw, cin).permute(0, 3, 1, 2).contiguous()
        return dx, dw, db, None, None, None, None


def conv2d(x, weight, bias=None, stride=1, padding=0, dilation=1, relu=False):
    """Differentiable `F.conv2d` (groups = 1, one stride for both directions, Cin % 32 == 0) on NCHW device tensors and an OIHW
    weight, optionally with the forward's fused ReLU.  The result is NCHW-shaped over channels-last memory."""
    hip._dev(x), hip._dev(weight)
    if bias is not None:
        hip._dev(bias)
    if x.dim() != 4 or weight.dim() != 4 or x.shape[1] != weight.shape[1]:
        raise hip.HipError('conv2d: input %s and weight %s do not fit' % (tuple(x.shape), tuple(weight.shape)))
    pad, dil = _pair(padding), _pair(dilation)
    if _wants_grad(x, weight, bias):
        return Conv2dFunction.apply(x, weight, bias, int(stride), pad, dil, bool(relu))
    return _conv2d_forward(x, weight, bias, int(stride), pad, dil, bool(relu))[2].permute(0, 3, 1, 2)


class BatchNormFunction(torch.autograd.Function):
    """y = [relu](batch_norm(x)) on an NCHW-shaped tensor; the kernels work on the NHWC map, which is what backward keeps
    (with the statistics the forward normalised with: the ReLU mask is recomputed from them, y is not saved)."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, training, momentum, eps, relu):
        xh = hip.to_nhwc(x.detach())
        w, b = weight.detach(), bias.detach()
        y, mean, invstd = hip.batch_norm_forward(xh, w, b, running_mean, running_var, training=training, momentum=momentum,
                                                 eps=eps, relu=relu)
        ctx.cfg = (training, eps, relu)
        if training:
            ctx.save_for_backward(xh, w, b, mean, invstd)
        else:
            ctx.save_for_backward(xh, w, b, running_mean, running_var)
        return y.permute(0, 3, 1, 2)

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        xh, w, b, s0, s1 = ctx.saved_tensors
        training, eps, relu = ctx.cfg
        saved = (s0, s1, None, None) if training else (None, None, s0, s1)
        dx, dw, db = hip.batch_norm_backward(hip.to_nhwc(dout), xh, w, b, *saved, training=training, eps=eps, relu=relu,
                                             need=ctx.needs_input_grad[:3])
        return (None if dx is None else dx.permute(0, 3, 1, 2)), dw, db, None, None, None, None, None, None


def batch_norm(x, weight, bias, running_mean, running_var, training, momentum=0.1, eps=1e-5, relu=False):
    """Differentiable `F.batch_norm` (affine, C % 4 == 0) on an NCHW device tensor, optionally with the ReLU behind it fused.
    The result is NCHW-shaped over channels-last memory; a channels-last input (what `conv2d` returns) is not copied.
    training: batch statistics, and running_mean / running_var (None = not tracked) move on the device whether or not a
    gradient is recorded.  Eval: the running statistics normalise."""
    hip._dev(x), hip._dev(weight), hip._dev(bias)
    if x.dim() != 4 or weight.dim() != 1 or x.shape[1] != weight.shape[0]:
        raise hip.HipError('batch_norm: input %s and weight %s do not fit' % (tuple(x.shape), tuple(weight.shape)))
    if not training and (running_mean is None or running_var is None):
        raise hip.HipError('batch_norm: eval mode needs the running statistics')
    args = (running_mean, running_var, bool(training), float(momentum), float(eps), bool(relu))
    if _wants_grad(x, weight, bias):
        return BatchNormFunction.apply(x, weight, bias, *args)
    y = hip.batch_norm_forward(hip.to_nhwc(x), weight.detach(), bias.detach(), running_mean, running_var, training=args[2],
                               momentum=args[3], eps=args[4], relu=args[5])[0]
    return y.permute(0, 3, 1, 2)


class BatchNormAddFunction(torch.autograd.Function):
    """y = [relu](batch_norm(x) + residual) on NCHW-shaped tensors; the kernels work on the NHWC maps.  Backward keeps x, the
    residual and the statistics the forward normalised with, and recomputes the mask of the sum from them: y is not saved."""

    @staticmethod
    def forward(ctx, x, residual, weight, bias, running_mean, running_var, training, momentum, eps, relu):
        xh, rh = hip.to_nhwc(x.detach()), hip.to_nhwc(residual.detach())
        w, b = weight.detach(), bias.detach()
        y, mean, invstd = hip.batch_norm_add_forward(xh, rh, w, b, running_mean, running_var, training=training,
                                                     momentum=momentum, eps=eps, relu=relu)
        ctx.cfg = (training, eps, relu)
        if training:
            ctx.save_for_backward(xh, rh, w, b, mean, invstd)
        else:
            ctx.save_for_backward(xh, rh, w, b, running_mean, running_var)
        return y.permute(0, 3, 1, 2)

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        xh, rh, w, b, s0, s1 = ctx.saved_tensors
        training, eps, relu = ctx.cfg
        saved = (s0, s1, None, None) if training else (None, None, s0, s1)
        nx, nr, nw, nb = ctx.needs_input_grad[:4]
        dx, dw, db, dr = hip.batch_norm_add_backward(hip.to_nhwc(dout), xh, rh, w, b, *saved, training=training, eps=eps,
                                                     relu=relu, need=(nx, nw, nb, nr))
        return ((None if dx is None else dx.permute(0, 3, 1, 2)), (None if dr is None else dr.permute(0, 3, 1, 2)), dw, db,
                None, None, None, None, None, None)


def batch_norm_add(x, residual, weight, bias, running_mean, running_var, training, momentum=0.1, eps=1e-5, relu=True):
    """Differentiable `relu(F.batch_norm(x) + residual)` (affine, C % 4 == 0; `relu=False`: the bare sum) on NCHW device tensors
    of one shape: the tail of a ResNet bottleneck as one kernel pair.  The result is NCHW-shaped over channels-last memory;
    channels-last inputs are not copied.  Statistics as in `batch_norm`: the residual does not enter them, and the running
    statistics move in training mode whether or not a gradient is recorded."""
    hip._dev(x), hip._dev(residual), hip._dev(weight), hip._dev(bias)
    if x.dim() != 4 or weight.dim() != 1 or x.shape[1] != weight.shape[0]:
        raise hip.HipError('batch_norm_add: input %s and weight %s do not fit' % (tuple(x.shape), tuple(weight.shape)))
    if residual.shape != x.shape:
        raise hip.HipError('batch_norm_add: residual %s does not belong to input %s' % (tuple(residual.shape), tuple(x.shape)))
    if not training and (running_mean is None or running_var is None):
        raise hip.HipError('batch_norm_add: eval mode needs the running statistics')
    args = (running_mean, running_var, bool(training), float(momentum), float(eps), bool(relu))
    if _wants_grad(x, residual, weight, bias):
        return BatchNormAddFunction.apply(x, residual, weight, bias, *args)
    y = hip.batch_norm_add_forward(hip.to_nhwc(x), hip.to_nhwc(residual), weight.detach(), bias.detach(), running_mean,
                                   running_var, training=args[2], momentum=args[3], eps=args[4], relu=args[5])[0]
    return y.permute(0, 3, 1, 2)


class ConfFusionFunction(torch.autograd.Function):
    """out[b] = sum_m exp(clamp(conf[b*M + m], -6, 4)) / S[b] * value[b*M + m] on NCHW-shaped tensors; the kernels work on the
    NHWC maps, which are all backward keeps: the weights and `out` are recomputed."""

    @staticmethod
    def forward(ctx, conf, value, batch, mem_size):
        ch, vh = hip.to_nhwc(conf.detach()), hip.to_nhwc(value.detach())
        ctx.bm = (batch, mem_size)
        ctx.save_for_backward(ch, vh)
        return hip.conf_fusion_forward(ch, vh, batch, mem_size).permute(0, 3, 1, 2)

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        ch, vh = ctx.saved_tensors
        dc, dv = hip.conf_fusion_backward(hip.to_nhwc(dout), ch, vh, *ctx.bm, need=ctx.needs_input_grad[:2])
        return (None if dc is None else dc.permute(0, 3, 1, 2)), (None if dv is None else dv.permute(0, 3, 1, 2)), None, None


def conf_fusion(conf, value, batch, mem_size):
    """Differentiable fusion of the reference's `Conf_Fusion.forward` behind its two conv - BN - ReLU branches: `conf` and
    `value` are NCHW-shaped device tensors [batch * mem_size, C, H, W] (C % 4 == 0), the result is [batch, C, H, W] over
    channels-last memory; a channels-last input (what `batch_norm` returns) is not copied."""
    hip._dev(conf), hip._dev(value)
    batch, mem_size = int(batch), int(mem_size)
    if conf.dim() != 4 or conf.shape != value.shape or conf.shape[0] != batch * mem_size:
        raise hip.HipError('conf_fusion: conf %s and value %s are not two [%d * %d, C, H, W] maps'
                           % (tuple(conf.shape), tuple(value.shape), batch, mem_size))
    if _wants_grad(conf, value):
        return ConfFusionFunction.apply(conf, value, batch, mem_size)
    return hip.conf_fusion_forward(hip.to_nhwc(conf.detach()), hip.to_nhwc(value.detach()), batch, mem_size).permute(0, 3, 1, 2)


class BoxExpFunction(torch.autograd.Function):
    """y = exp(adjust * p + bias[c]) on an NCHW-shaped [N, 4, H, W] tensor; adjust and bias stay on the device.  Backward keeps
    the NHWC map of p and the two parameters; y is recomputed."""

    @staticmethod
    def forward(ctx, p, adjust, bias):
        ph, a, b = hip.to_nhwc(p.detach()), adjust.detach(), bias.detach()
        ctx.save_for_backward(ph, a, b)
        return hip.box_exp_forward(ph, a, b).permute(0, 3, 1, 2)

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        ph, a, b = ctx.saved_tensors
        dp, da, db = hip.box_exp_backward(hip.to_nhwc(dy), ph, a, b, need=ctx.needs_input_grad[:3])
        return (None if dp is None else dp.permute(0, 3, 1, 2)), da, db


def box_exp(p, adjust, bias):
    """Differentiable `torch.exp(adjust * p + bias)` of the reference's box head: `p` an NCHW-shaped device tensor [N, 4, H, W]
    (the `bbox_pred` output; a channels-last one is not copied), `adjust` one float, `bias` four ([1, 4, 1, 1]).  The result is
    NCHW-shaped over channels-last memory."""
    hip._dev(p), hip._dev(adjust), hip._dev(bias)
    if p.dim() != 4 or p.shape[1] != 4 or adjust.numel() != 1 or bias.numel() != 4:
        raise hip.HipError('box_exp: p %s, adjust %s and bias %s are not [N, 4, H, W], one float and four'
                           % (tuple(p.shape), tuple(adjust.shape), tuple(bias.shape)))
    if _wants_grad(p, adjust, bias):
        return BoxExpFunction.apply(p, adjust, bias)
    return hip.box_exp_forward(hip.to_nhwc(p.detach()), adjust.detach(), bias.detach()).permute(0, 3, 1, 2)
