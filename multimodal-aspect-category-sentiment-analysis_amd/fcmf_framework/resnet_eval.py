"""Eval-mode ResNet trunk with BatchNorm folded into the convolutions (inference: predict.py).

In eval() mode a BatchNorm2d is the per-channel affine z = s * y + t with s = gamma / sqrt(running_var + eps) and
t = beta - running_mean * s.  `FoldedTrunk(net)` snapshots a `resnet.ResNet` once: s goes into the convolution's weight rows
(W' = s[:, None] * W, formed in float32 and cast ONCE to the compute dtype), t stays a float32 bias, and ReLU / the bottleneck's
residual add ride in the GEMM epilogue (FCMF_EPI_RELU / FCMF_EPI_ADD_RELU).  Per bottleneck (bf16, power-of-two widths >= 64):

    conv1       GEMM + bias, then fcmf_bn_apply_pad (unit scale, zero shift, relu) into the zero-bordered input of the 3x3
    conv2       fcmf_conv_gemm_epi, EPI_RELU                                   one launch
    downsample  GEMM / fcmf_conv_gemm_epi (strided), bias only
    conv3       GEMM, EPI_ADD_RELU with aux = the identity                     one launch

Other dtypes / widths (float32, the tiny trunks of the tests): conv1 = GEMM with EPI_RELU, conv2 / strided shortcut = patch matrix
(fcmf_conv_im2col) + GEMM with the same epilogues.  The stem keeps resnet.conv2d_stem / conv2d_nhwc on the module's own weight
plus one fcmf_bn_apply pass with (s, t).  No statistics launch (fcmf_bn_stats*, fcmf_bn_finalize*) exists on this path.

The snapshot is explicit: it does not go through the version-keyed shadow cache (BatchNorm buffers changing under an unchanged
convolution weight would leave a stale entry there); `refresh()` rebuilds it after the module's parameters or buffers changed.
(One change it learns of by itself: `FusedAdamW.ema_weights()` exchanging parameters and averaged weights counts `shadows.swaps`
up, and a call that finds the count moved since the snapshot takes a new one first.)
`resnet.Bottleneck.run`, `ResNet._trunk_pass` and `trunk_nhwc` are untouched: this is a second, opt-in walk.
"""
import torch

from . import _hip as H
from . import ops
from . import resnet as R


class _Stage:
    """one conv -> bn pair, folded: wm [Cout, Kpad] (compute dtype, k = (r, s, c), zero tail), bias float32 [Cout]"""
    __slots__ = ("conv", "wm", "bias", "Kpad")

    def __init__(self, conv, bn, dtype):
        if conv.bias is not None or conv.groups != 1 or conv.dilation != (1, 1):
            raise H.HipLibraryError("FoldedTrunk: bias-free, ungrouped, undilated convolutions only (ResNet trunk)")
        s, t = _affine(bn)
        w = conv.weight.detach().float() * s[:, None, None, None]
        Cout, Cin, kh, kw = w.shape
        K = kh * kw * Cin
        self.Kpad = (K + 31) // 32 * 32
        m = w.permute(0, 2, 3, 1).reshape(Cout, K)
        if self.Kpad != K:
            m = torch.cat((m, m.new_zeros(Cout, self.Kpad - K)), 1)
        self.conv, self.wm, self.bias = conv, ops.cast(m.contiguous(), dtype), t.contiguous()


def _affine(bn):
    """(s, t) float32 of an eval-mode BatchNorm2d"""
    g = bn.weight.detach().float() if bn.weight is not None else torch.ones_like(bn.running_var, dtype=torch.float32)
    b = bn.bias.detach().float() if bn.bias is not None else torch.zeros_like(g)
    s = g / torch.sqrt(bn.running_var.detach().float() + float(bn.eps))
    return s, b - bn.running_mean.detach().float() * s


class FoldedTrunk:
    def __init__(self, net):
        if not isinstance(net, R.ResNet):
            raise H.HipLibraryError("FoldedTrunk: a fcmf_framework.resnet.ResNet is required (resnet.from_module converts others)")
        self.net = net
        self.refresh()

    def refresh(self):
        """rebuild the snapshot from the module's current parameters and running statistics"""
        net = self.net
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d) and (m.training or not m.track_running_stats or m.running_mean is None):
                raise H.HipLibraryError("FoldedTrunk: the network must be in eval() mode with tracked running statistics "
                                        "(train-mode BatchNorm normalises with batch statistics: nothing to fold)")
        H.require_cuda(net.conv1.weight)
        self.dtype = dt = ops.compute_dtype()
        self._swaps = ops.shadows.swaps
        with torch.no_grad():
            self.stem_scale, self.stem_shift = (v.contiguous() for v in _affine(net.bn1))
            self.blocks = []
            for layer in (net.layer1, net.layer2, net.layer3, net.layer4):
                for b in layer:
                    down = _Stage(b.downsample[0], b.downsample[1], dt) if b.downsample is not None else None
                    self.blocks.append((_Stage(b.conv1, b.bn1, dt), _Stage(b.conv2, b.bn2, dt), _Stage(b.conv3, b.bn3, dt), down))
            dev = net.conv1.weight.device
            self._unit = {}       # C -> (ones, zeros): the unit affine of the relu + pad pass
            for s1, _, _, _ in self.blocks:
                C = s1.conv.out_channels
                if C not in self._unit:
                    self._unit[C] = (torch.ones(C, dtype=torch.float32, device=dev), torch.zeros(C, dtype=torch.float32, device=dev))
        return self

    # ---- stages ---------------------------------------------------------------------------------------------------------
    @staticmethod
    def _gemm(A, st, rows, epi, aux=None):
        """A [rows, Kpad] . wm^T + bias (+ aux) (relu) -> [rows, Cout]"""
        Cout = st.conv.out_channels
        y = torch.empty((rows, Cout), dtype=A.dtype, device=A.device)
        ops.gemm(A, st.wm, y, rows, Cout, st.Kpad, st.Kpad, st.Kpad, Cout, 0, 0, bias=st.bias, aux=aux, epi=epi)
        return y

    def _conv(self, x, st, epi, aux=None, xp=None):
        """x [N, H, W, C] -> [N, Ho, Wo, Cout] = epi(conv(x, W') + t (+ aux)).  xp: x with the convolution's zero border already in
        place (the implicit-GEMM input); else 1x1 / stride 1 reads x in place, strided 1x1 is gathered by the implicit GEMM where the
        shape allows, and everything else goes through a patch matrix."""
        conv = st.conv
        kh, kw = conv.kernel_size
        sd, pad, Cout = conv.stride[0], conv.padding[0], conv.out_channels
        N, Hh, Ww, C = x.shape if xp is None else (xp.shape[0], xp.shape[1] - 2 * pad, xp.shape[2] - 2 * pad, xp.shape[3])
        Ho, Wo = (Hh + 2 * pad - kh) // sd + 1, (Ww + 2 * pad - kw) // sd + 1
        rows = N * Ho * Wo
        a2 = aux.view(rows, Cout) if aux is not None else None
        src = xp if xp is not None else x
        if xp is not None or (kh == 1 and kw == 1 and pad == 0 and sd > 1 and R._implicit_ok(C, x.dtype)):
            y = torch.empty((rows, Cout), dtype=src.dtype, device=src.device)
            with ops.trace_launch(2.0 * rows * Cout * st.Kpad) as t:
                rc = H.lib().fcmf_conv_gemm_epi(H.gemm_ctx(), H.ptr(src), H.ptr(st.wm), H.ptr(y), H.ptr(st.bias), H.ptr(a2), epi,
                                                N, src.shape[1], src.shape[2], C, Ho, Wo, kh, kw, sd, Cout, H.stream())
                if rc != 0:
                    t.flops = None
            H.check(rc, "fcmf_conv_gemm_epi")
            return y.view(N, Ho, Wo, Cout)
        if kh == 1 and kw == 1 and sd == 1 and pad == 0 and C == st.Kpad and x.dtype == self.dtype and x.is_contiguous():
            A = x.view(rows, C)       # read in place: the GEMM contracts over Kpad = C columns of a dense activation
        else:                         # (also a width that is no multiple of 32: the patch matrix carries the zero tail)
            A = torch.empty((rows, st.Kpad), dtype=self.dtype, device=x.device)
            sn, sh, sw, sc = x.stride()
            H.check(H.lib().fcmf_conv_im2col(H.ptr(x), H.dt(x), H.ptr(A), H.dt(A), N, Hh, Ww, C, sn, sh, sw, sc, kh, kw, sd, pad,
                                             st.Kpad, H.stream()), "fcmf_conv_im2col")
        return self._gemm(A, st, rows, epi, a2).view(N, Ho, Wo, Cout)

    def _block(self, x, stages):
        s1, s2, s3, down = stages
        N, Hh, Ww, _ = x.shape
        C = s1.conv.out_channels
        if R._implicit_ok(C, x.dtype):
            # conv1 + bias, then relu into the zero-bordered input of the 3x3 convolution (the block's one apply-type launch)
            y1 = self._conv(x, s1, H.EPI_NONE)
            zp = R.padded_activation(N, Hh, Ww, C, x.dtype, x.device)
            one, zero = self._unit[C]
            H.check(H.lib().fcmf_bn_apply_pad(H.ptr(y1), 0, H.ptr(zp), H.ptr(one), H.ptr(zero), N * Hh * Ww, C, N * Hh * Ww, 1, Hh, Ww, 1,
                                              H.dt(y1), H.stream()), "fcmf_bn_apply_pad")
            z2 = self._conv(None, s2, H.EPI_RELU, xp=zp)
        else:
            z2 = self._conv(self._conv(x, s1, H.EPI_RELU), s2, H.EPI_RELU)
        idn = x if down is None else self._conv(x, down, H.EPI_NONE)
        return self._conv(z2, s3, H.EPI_ADD_RELU, aux=idn)

    def _pass(self, x):
        net = self.net
        xs = x if x.dtype in (torch.float32, torch.bfloat16) else x.float()
        v = xs.permute(0, 2, 3, 1)                                       # strided NHWC view of the NCHW crops
        if R._stem_runs_ok(net.conv1, v, self.dtype):
            y = R.conv2d_stem(v, net.conv1)
        else:
            y = R.conv2d_nhwc(v, net.conv1, src_strides=v.stride())
        N, Hh, Ww, C = y.shape
        H.check(H.lib().fcmf_bn_apply(H.ptr(y), 0, H.ptr(y), H.ptr(self.stem_scale), H.ptr(self.stem_shift), N * Hh * Ww, C, N * Hh * Ww, 1,
                                      H.dt(y), H.stream()), "fcmf_bn_apply")
        y = R.maxpool3x3s2_nhwc(y)
        for stages in self.blocks:
            y = self._block(y, stages)
        return y

    def __call__(self, x):
        """x [N, 3, H, W] (any float dtype / layout) -> NHWC [N, h, w, C], detached"""
        H.require_cuda(x)
        if self._swaps != ops.shadows.swaps:
            self.refresh()        # FusedAdamW.ema_weights() exchanged the weights since the snapshot (it cannot mark this copy stale)
        if ops.compute_dtype() != self.dtype:
            raise H.HipLibraryError(f"FoldedTrunk: snapshot taken in {self.dtype}, compute dtype is now {ops.compute_dtype()}: call refresh()")
        with torch.no_grad():
            outs = [self._pass(x[i:i + R.MAX_CROPS_PER_PASS]) for i in range(0, x.shape[0], R.MAX_CROPS_PER_PASS)]
        return outs[0] if len(outs) == 1 else torch.cat(outs, 0)
