"""What the convolution + BatchNorm plans share (ChangeFormer's decoder, Unet / BIT-CD on ResNet-18, FC-Siam): the convolution and
weight-gradient builders over ksmi_conv_forward / ksmi_conv_wgrad, the BatchNorm forward / backward forms, the epilogue masks, the
gradient-buffer bookkeeping of the closure-built backward pass and the class-map head."""
import ctypes as C
import os

import torch

from .plan_base import PlanBase
from .runtime import SrcSpec, conv_grid_m, conv_stats_rows, make_conv, make_wgrad

BN_EPS, BN_MOMENTUM = 1e-5, 0.1
CS = 8            # channel stride of the 3-channel NHWC heads (vector-aligned pad channels)


def drop_threshold(p):
    """(thr, inv_keep): an element is dropped when its 32-bit draw < thr = round(p * 2^32); kept ones are scaled by 1/(1-p)"""
    if p <= 0.0:
        return 0, 1.0
    if p >= 1.0:
        raise ValueError("drop probability must be < 1")
    return min(0xFFFFFFFF, int(round(p * 4294967296.0))), 1.0 / (1.0 - p)


class ConvPlan(PlanBase):
    def _init_conv(self, model, B, H, W, dtype, training, with_backward, const_width=512):
        self._init_base(model, dtype, with_backward)
        self.B, self.H, self.W, self.training = B, H, W, training
        self.const = torch.zeros((2, const_width), dtype=torch.float32, device=self.dev)   # row 0 zeros, row 1 ones
        self.const[1].fill_(1.0)
        self._gbuf = {}            # id(tensor) -> gradient buffer ; first writer "=", later writers "+="
        self._gacc = set()
        self._bwd = []             # backward closures, appended in forward order

    def _build_lists(self, build):
        """the forward graph, then the backward closures it left behind (last first), then scratch and pack table"""
        build()
        if self.with_backward:
            for f in reversed(self._bwd):
                f()
        self._finish()

    @property
    def _bn_fused(self):
        """BatchNorm partial rows finish inside the apply pass (bnfused.hip, as in the SNUNet plan since round 4): one launch less per
        BatchNorm; KSMI_BN_FUSED_FAMILIES=0 keeps the separate finalize / reduce_rows launch (A/B)"""
        return os.environ.get("KSMI_BN_FUSED_FAMILIES", "1") != "0"

    # ---------------------------------------------------------------- gradient bookkeeping
    def gbuf(self, t):
        if id(t) not in self._gbuf:
            self._gbuf[id(t)] = self.buf(*t.shape)
        return self._gbuf[id(t)]

    def gacc(self, t):
        """accumulate flag for the next writer of d(t): 0 for the first one"""
        a = 1 if id(t) in self._gacc else 0
        self._gacc.add(id(t))
        return a

    def _zero_grad_key(self, key):
        g = self.m._g(key)
        self._pinit.add(key)
        self.bwd.add("ksmi_fill_zero", lambda: (g.data_ptr(), g.numel() * 4))
        self._mark(key)

    # ---------------------------------------------------------------- epilogue masks
    def _nomask(self, r, sv):
        """epilogue 'mask' tuple that only accumulates the BatchNorm-backward sums (sum dy, sum dy*rhat) without masking"""
        return (r, sv.t[0], sv.t[1], self.const[0], self.const[1])

    def _relumask(self, r):
        return (r, self.const[0], self.const[1], self.const[1], self.const[0])

    def _bnmask(self, z, sv):
        """epilogue mask of a consumer's input gradient: ReLU(bn(z)) active set + BatchNorm-backward sums"""
        return (z, sv.t[0], sv.t[1], sv.t[2], sv.t[3])

    # ---------------------------------------------------------------- convolutions
    def _attach_stats(self, d, offset=0):
        """BatchNorm sums from the epilogue of descriptor d into scratch 'stats' (+ offset bytes) -> its statistics rows"""
        # statistics rows of the kernel that will run this descriptor (one per persistent workgroup on igemm3 / igemm4, one per M-tile on
        # igemm2; recorded in d.stats_rows: with the tile kernel's count the dispatch kept every convolution WITH statistics off the ring
        # kernel -- diff_c1.0 ran at 660 instead of ~1100 TFLOP/s until round 5)
        rows = conv_stats_rows(d, self.dtype)
        self.need("stats", offset + rows * 2 * d.Npad * 4)
        self._later.append(lambda: setattr(d, "stats", self.scr("stats") + offset))
        return rows

    def _cv(self, ll, name, srcs, dsts, wkey, Hin, Win, Hout, Wout, k, stride, pad, N, Ktot, stats=False, mask=None, bkey=None, tag="conv",
            relu_out=0, alpha=0.0, resid=None, dgrad=False, B=None):
        """k x k convolution -> (statistics rows, padded columns).  dgrad=True packs W for the input gradient (K = output channels,
        flipped taps)."""
        d, table = make_conv(srcs, dsts, dsts[0][0], self.m._p(bkey) if bkey else None, None, self.B if B is None else B, Hin, Win, Hout, Wout,
                             k, k, stride, pad, N, self.dtype, mask=mask, alpha=alpha, relu_out=relu_out, resid=resid)
        taps = k * k
        if dgrad:      # element (k = n_out, tap', col = c_in) = W[n][c][flip(tap')]
            d.wpk = self._packed(wkey, table, taps, N, N, N * taps, taps, 0, 1, 1).data_ptr()
        else:          # element (k = c_in, tap, col = n_out) = W[n][c][tap]
            d.wpk = self._packed(wkey, table, taps, N, N, taps, Ktot * taps, 0, 1, 0).data_ptr()
        rows = self._attach_stats(d) if stats else conv_grid_m(d)
        self._conv(ll, d, f"{tag}{k}x{k}" + ("_dgrad" if dgrad else ""), name)
        return rows, d.Npad

    def _conv3(self, ll, name, srcs, dsts, wkey, bkey, B, H, W, N, Ktot, **kw):
        """3x3 s1 p1 convolution"""
        return self._cv(ll, name, srcs, dsts, wkey, H, W, H, W, 3, 1, 1, N, Ktot, bkey=bkey, B=B, **kw)

    def _wg(self, srcs, dy, N, wkey, Hin, Win, Hout, Wout, k, stride, pad, Ktot):
        taps = k * k
        dw, ws = make_wgrad(srcs, dy, N, 0, N, self.m._g(wkey), taps, Ktot * taps, 1, self._acc_param(wkey), self.B, Hin, Win, Hout, Wout,
                            k, k, stride, pad, self.dtype)
        self._wgrad(dw, ws, wkey)

    # ---------------------------------------------------------------- BatchNorm
    def _stats_ptr(self):
        return (lambda: self.scr("stats")) if self.training else (lambda: None)

    def _bn_finalize(self, key, sv, rows, cpad, Cc, count):
        m, tr = self.m, self.training
        g, b = m._p(f"{key}.weight").data_ptr(), m._p(f"{key}.bias").data_ptr()
        rm, rv, nbt = m._b(f"{key}.running_mean").data_ptr(), m._b(f"{key}.running_var").data_ptr(), m._c(f"{key}.num_batches_tracked").data_ptr()
        st = self._stats_ptr()
        self.fwd.add("ksmi_bn_finalize", lambda: (st(), rows, cpad, Cc, float(count), g, b, rm, rv, nbt, BN_MOMENTUM, BN_EPS,
                                                  1 if tr else 0, sv.mean, sv.rstd, sv.scale, sv.shift))

    def _affine(self, ll, x, sv, y, npix, Cc, relu):
        dt = self.dt
        ll.add("ksmi_affine", lambda: (x.data_ptr(), sv.scale, sv.shift, y.data_ptr(), npix, Cc, relu, C.c_float(1.0), dt),
               self._elt_meta("bn_apply", 2 * npix * Cc))

    def _bn_bwd_args(self, key, Cc, npix=None):
        """what the BatchNorm-backward forms share -> (partial rows of an own reduce pass over npix pixels, dgamma, dbeta, their
        accumulate flag, gamma)"""
        rows = None
        if npix is not None:
            rows = max(1, min(512, npix // 256))
            self.need("bnp", rows * 2 * Cc * 4)
        self.need("bnsum", 2 * Cc * 4)
        gw, gb = self.m._g(f"{key}.weight").data_ptr(), self.m._g(f"{key}.bias").data_ptr()
        a1, _ = self._acc_param(f"{key}.weight"), self._acc_param(f"{key}.bias")
        return rows, gw, gb, a1, self.m._p(f"{key}.weight").data_ptr()

    def _bn_backward(self, key, dy, r, sv, dv, rows, cpad, Cc, count, npix, relu_mask):
        """sums (from the consumer's dgrad epilogue in scratch 'stats') -> dgamma, dbeta, dv"""
        _, gw, gb, a1, gamma = self._bn_bwd_args(key, Cc)
        # (fused form, _bn_fused: only where the gradient arrives already masked, bnfused.hip MODE 0)
        if relu_mask == 0 and self._bn_fused and self.lib.ksmi_bn_fused_supported(Cc, cpad, self.dt):
            self.bwd.add("ksmi_bn_bwd_fin_apply_gated", lambda: (self.scr("stats"), rows, cpad, self.scr("bnsum"), gw, gb, a1, dy.data_ptr(), r.data_ptr(),
                                                                 sv.mean, sv.rstd, gamma, dv.data_ptr(), float(count), npix, Cc, self.dt),
                         self._elt_meta("bn_bwd_apply", 3 * npix * Cc))
            self._mark(f"{key}.weight", f"{key}.bias")
            return
        self.bwd.add("ksmi_reduce_rows", lambda: (self.scr("stats"), rows, 2, cpad, Cc, self.scr("bnsum"), gw, gb, a1))
        self._mark(f"{key}.weight", f"{key}.bias")
        self.bwd.add("ksmi_bn_bwd_apply", lambda: (dy.data_ptr(), r.data_ptr(), sv.mean, sv.rstd, gamma, self.scr("bnsum"), dv.data_ptr(),
                                                   relu_mask, float(count), npix, Cc, self.dt), self._elt_meta("bn_bwd_apply", 3 * npix * Cc))

    def _bnrelu_bwd(self, bnkey, dout, out, z, sv, dz, npix, Cc, alpha=None):
        """out = relu(bn(z) [+ identity]) materialised: dout -> g (in place), dz, dgamma, dbeta.
        alpha (FC-Siam): out = relu(bn(z)) * Dropout2d; the plane scale 1/(1-p) is constant on the active set (read from out > 0),
        so the BatchNorm + ReLU backward kernels run unchanged and alpha scales dz, dgamma, dbeta"""
        rows, gw, gb, a1, gamma = self._bn_bwd_args(bnkey, Cc, npix)
        dt = self.dt
        self.bwd.add("ksmi_bnrelu_bwd_reduce", lambda: (dout.data_ptr(), out.data_ptr(), z.data_ptr(), sv.mean, sv.rstd, self.scr("bnp"), rows, npix, Cc, dt),
                     self._elt_meta("bnrelu_bwd_reduce", 3 * npix * Cc))
        if alpha is not None:
            alpha = C.c_float(alpha)
            self.bwd.add("ksmi_reduce_rows_scaled", lambda: (self.scr("bnp"), rows, 2, Cc, Cc, self.scr("bnsum"), gw, gb, a1, alpha))
            self._mark(f"{bnkey}.weight", f"{bnkey}.bias")
            self.bwd.add("ksmi_bnrelu_bwd_apply_scaled", lambda: (dout.data_ptr(), out.data_ptr(), z.data_ptr(), sv.mean, sv.rstd, gamma, self.scr("bnsum"),
                                                                  dz.data_ptr(), float(npix), npix, Cc, alpha, dt),
                         self._elt_meta("bnrelu_bwd_apply", 5 * npix * Cc))
            return
        if self._bn_fused and self.lib.ksmi_bn_fused_supported(Cc, Cc, dt):
            self.bwd.add("ksmi_bnrelu_bwd_fin_apply", lambda: (self.scr("bnp"), rows, Cc, self.scr("bnsum"), gw, gb, a1, dout.data_ptr(), out.data_ptr(),
                                                               z.data_ptr(), sv.mean, sv.rstd, gamma, dz.data_ptr(), float(npix), npix, Cc, dt),
                         self._elt_meta("bnrelu_bwd_apply", 5 * npix * Cc))
            self._mark(f"{bnkey}.weight", f"{bnkey}.bias")
            return
        self.bwd.add("ksmi_reduce_rows", lambda: (self.scr("bnp"), rows, 2, Cc, Cc, self.scr("bnsum"), gw, gb, a1))
        self._mark(f"{bnkey}.weight", f"{bnkey}.bias")
        self.bwd.add("ksmi_bnrelu_bwd_apply", lambda: (dout.data_ptr(), out.data_ptr(), z.data_ptr(), sv.mean, sv.rstd, gamma, self.scr("bnsum"), dz.data_ptr(),
                                                       float(npix), npix, Cc, dt), self._elt_meta("bnrelu_bwd_apply", 5 * npix * Cc))

    def _bn_plain_bwd(self, bnkey, dy, x, sv, dv, npix, Cc):
        rows, gw, gb, a1, gamma = self._bn_bwd_args(bnkey, Cc, npix)
        dt = self.dt
        self.bwd.add("ksmi_bn_bwd_reduce", lambda: (dy.data_ptr(), x.data_ptr(), sv.mean, sv.rstd, self.scr("bnp"), rows, npix, Cc, dt),
                     self._elt_meta("bn_bwd_reduce", 2 * npix * Cc))
        self.bwd.add("ksmi_reduce_rows", lambda: (self.scr("bnp"), rows, 2, Cc, Cc, self.scr("bnsum"), gw, gb, a1))
        self._mark(f"{bnkey}.weight", f"{bnkey}.bias")
        self.bwd.add("ksmi_bn_bwd_apply", lambda: (dy.data_ptr(), x.data_ptr(), sv.mean, sv.rstd, gamma, self.scr("bnsum"), dv.data_ptr(), 0, float(npix),
                                                   npix, Cc, dt), self._elt_meta("bn_bwd_apply", 3 * npix * Cc))

    # ---------------------------------------------------------------- |s1 - s2|
    def _absdiff(self, s1, s2, Cc, h, w):
        B, dt = self.B, self.dt
        n = B * h * w * Cc
        dbuf = self.buf(B, h, w, Cc)
        self.fwd.add("ksmi_absdiff_forward", lambda: (s1.data_ptr(), s2.data_ptr(), dbuf.data_ptr(), n, dt), self._elt_meta("absdiff", 3 * n))

        def bwd():
            dd, d1, d2 = self.gbuf(dbuf), self.gbuf(s1), self.gbuf(s2)
            a1, a2 = self.gacc(s1), self.gacc(s2)
            self.bwd.add("ksmi_absdiff_backward", lambda: (s1.data_ptr(), s2.data_ptr(), dd.data_ptr(), d1.data_ptr(), d2.data_ptr(), a1, a2, n, dt),
                         self._elt_meta("absdiff_bwd", 5 * n))
        self._bwd.append(bwd)
        return dbuf

    # ---------------------------------------------------------------- class-map head (3x3 convolution onto the CS-strided map), backward
    def _class_dP(self, act):
        """gradient of the class map from self.dlogits (through the output activation `act`) -> (dP, dP as a convolution source)"""
        B, HW, nc = self.B, self.H * self.W, self.nc
        dP = self.buf(B * HW, CS)
        self.bwd.add("ksmi_dout_to_nhwc", lambda: (self.dlogits.data_ptr(), self.logits.data_ptr(), dP.data_ptr(), B, nc, CS, HW, act, self.dt))
        return dP, [SrcSpec(dP, CS, 0, CS, k_real=nc)]

    def _class_bias_bwd(self, dP, bk):
        B, HW, nc, dt = self.B, self.H * self.W, self.nc, self.dt
        rr = max(1, min(512, B * HW // 256))
        self.need("red", rr * CS * 4)
        accb = self._acc_param(bk)
        gb = self.m._g(bk).data_ptr()
        self.bwd.add("ksmi_channel_sum", lambda: (dP.data_ptr(), self.scr("red"), rr, B * HW, CS, dt), self._elt_meta("channel_sum", B * HW * CS))
        self.bwd.add("ksmi_reduce_rows", lambda: (self.scr("red"), rr, 1, CS, nc, None, None, gb, accb))
        self._mark(bk)

    def _class_head_bwd(self, name, wk, bk, y, Cy):
        """backward of P = conv3x3(y) + b, logits = NCHW(P): -> d(y) (first writer); dW via the operand swap (halo side = dP):
        G[tap][o][c] = dW[o][c][8 - tap]"""
        B, H, W, nc = self.B, self.H, self.W, self.nc
        dy = self.gbuf(y)
        self.gacc(y)
        dP, psrc = self._class_dP(0)
        self._conv3(self.bwd, name, psrc, [(dy, Cy, 0, 0, Cy, 0)], wk, None, B, H, W, Cy, nc, dgrad=True)
        gview = self.m._g(wk)[8:]
        self.keep.append(gview)
        dw, ws = make_wgrad(psrc, y, Cy, 0, Cy, gview, Cy * 9, 9, -1, self._acc_param(wk), B, H, W, H, W, 3, 3, 1, 1, self.dtype)
        self._wgrad(dw, ws, wk)
        self._class_bias_bwd(dP, bk)
        return dy
