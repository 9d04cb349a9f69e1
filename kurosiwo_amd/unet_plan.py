"""Static launch plan of one Unet(resnet18) forward/backward (row U1 of SURVEY.md §8(a)); architecture: oracle/unet_ref.py.

conv -> BatchNorm -> ReLU chains never materialise the normalised tensor when the consumer is a convolution (BN-apply + ReLU on the
operand load; the consumer's input-gradient epilogue applies the ReLU mask and accumulates the BN-backward sums); tensors that feed
pooling / upsampling / skip concatenation / the residual sum are materialised once.  Strided 3x3 and 1x1 convolutions get their
input gradients as phase convolutions written through the strided output placement of the implicit-GEMM kernel.
"""
import os

import torch

from . import _lib
from .conv_plan import BN_EPS, BN_MOMENTUM, CS, ConvPlan
from .runtime import SrcSpec, conv_grid_m, make_conv, phase_taps_k3s2
from .plan_base import _Saved
from .unet import DECODER_CHANNELS, LAYERS


class ResNetPlan(ConvPlan):
    """torchvision ResNet-18 pieces shared by the Unet encoder and BIT-CD's siamese backbone: stem and BasicBlock"""
    side_wgrad = True          # plan_base.PlanBase.side_wgrad: dedicated buffers throughout (self.buf), conv weight gradients only

    def _dgrad_s2(self, name, dy, Cout, dx, Cin, H, W, wkey, acc):
        """input gradient of a 3x3 stride-2 pad-1 convolution: four 2x2 phase convolutions over dy (runtime.phase_taps_k3s2)"""
        Ho, Wo = H // 2, W // 2
        for py in range(2):
            for px in range(2):
                d, table = make_conv([SrcSpec(dy, Cout)], [(dx, Cin, 0, 0, Cin, acc)], dx, None, None, self.B, Ho, Wo, Ho, Wo, 2, 2, 1, 0, Cin,
                                     self.dtype, out_map=(2, 2, py, px, H, W))
                d.wpk = self._packed(wkey, table, 4, Cin, Cin, Cin * 9, 9, 0, 1, 0, phase_taps_k3s2(py, px)).data_ptr()
                self._conv(self.bwd, d, "dgrad_s2_phase", f"{name}.p{py}{px}")

    # ---------------------------------------------------------------- conv1 7x7 s2 -> bn1 -> relu -> maxpool 3x3 s2
    def _resnet_stem(self, prefix, x):
        """x: fp32 NCHW input tile -> (stem output before the pool, pooled output, its height, width)"""
        B, H, W, dt = self.B, self.H, self.W, self.dt
        H1, W1 = H // 2, W // 2
        R1 = B * H1 * W1
        kc = 32 if self.dtype == torch.bfloat16 else 16
        Kreal = self.cin * 49
        Kpad = -(-Kreal // kc) * kc
        col, s0, f1 = self.buf(R1, Kpad), self.buf(R1, 64), self.buf(B, H1, W1, 64)
        sv0 = _Saved(64, self.dev)
        self.fwd.add("ksmi_im2col", lambda: (x.data_ptr(), col.data_ptr(), B, self.cin, H, W, H1, W1, 7, 7, 2, 3, Kpad, 1, dt),
                     self._elt_meta("im2col", 2 * R1 * Kpad))
        d, table = make_conv([SrcSpec(col, Kpad, k_real=Kreal)], [(s0, 64, 0, 0, 64, 0)], s0, None, None, 1, R1, 1, R1, 1, 1, 1, 1, 0, 64, self.dtype)
        d.wpk = self._packed(f"{prefix}.conv1.weight", table, 1, 64, 64, 1, Kreal, 0, 0).data_ptr()
        rows0 = self._attach_stats(d) if self.training else conv_grid_m(d)
        self._conv(self.fwd, d, "stem7x7", f"{prefix}.conv1")
        self._bn_finalize(f"{prefix}.bn1", sv0, rows0, d.Npad, 64, R1)
        self._affine(self.fwd, s0, sv0, f1, R1, 64, 1)
        H2, W2 = H1 // 2, W1 // 2
        p = self.buf(B, H2, W2, 64)
        # with a backward pass the forward records the window position of each first maximum (one byte per output element): the backward
        # compares codes instead of re-reading up to four windows per input element (325 -> ~40 us at 112 x 112 x 64 x 32 images)
        pidx = torch.empty(p.numel(), dtype=torch.uint8, device=self.dev) if self.with_backward and not os.environ.get("KSMI_MAXPOOL_GATHER") else None
        if pidx is not None:
            self.fwd.add("ksmi_maxpool3x3s2_forward_idx", lambda: (f1.data_ptr(), p.data_ptr(), pidx.data_ptr(), B, H1, W1, 64, dt),
                         self._elt_meta("maxpool3", 2 * R1 * 64))
        else:
            self.fwd.add("ksmi_maxpool3x3s2_forward", lambda: (f1.data_ptr(), p.data_ptr(), B, H1, W1, 64, dt), self._elt_meta("maxpool3", 2 * R1 * 64))

        def bwd():
            df1, ds0 = self.gbuf(f1), self.buf(R1, 64)
            dp = self.gbuf(p)
            acc = self.gacc(f1)
            if pidx is not None:
                self.bwd.add("ksmi_maxpool3x3s2_backward_idx", lambda: (pidx.data_ptr(), dp.data_ptr(), df1.data_ptr(), acc, B, H1, W1, 64, dt),
                             self._elt_meta("maxpool3_bwd", 2 * R1 * 64 + R1 * 64 // 2 + R1 * 64 // 4))
            else:
                self.bwd.add("ksmi_maxpool3x3s2_backward", lambda: (f1.data_ptr(), dp.data_ptr(), df1.data_ptr(), acc, B, H1, W1, 64, dt),
                             self._elt_meta("maxpool3_bwd", 4 * R1 * 64))
            self._bnrelu_bwd(f"{prefix}.bn1", df1, f1, s0, sv0, ds0, R1, 64)
            self._linear_bwd(f"{prefix}.conv1", col, Kpad, f"{prefix}.conv1.weight", None, ds0, 64, R1, None, k_real=Kreal)
        self._bwd.append(bwd)
        return f1, p, H2, W2

    # ---------------------------------------------------------------- BasicBlock (torchvision resnet.py)
    def _basic_block(self, k, x_in, Cin, Cout, H, W, stride):
        B, dt = self.B, self.dt
        Ho, Wo = H // stride, W // stride
        npix = B * Ho * Wo
        i1, z2, out = self.buf(B, Ho, Wo, Cout), self.buf(B, Ho, Wo, Cout), self.buf(B, Ho, Wo, Cout)
        sv1, sv2 = _Saved(Cout, self.dev), _Saved(Cout, self.dev)
        rows, cpad = self._cv(self.fwd, f"{k}.conv1", [SrcSpec(x_in, Cin)], [(i1, Cout, 0, 0, Cout, 0)], f"{k}.conv1.weight", H, W, Ho, Wo, 3, stride, 1,
                              Cout, Cin, stats=self.training)
        self._bn_finalize(f"{k}.bn1", sv1, rows, cpad, Cout, npix)
        a1 = [SrcSpec(i1, Cout, scale=sv1.scale_t, shift=sv1.shift_t, relu=1)]
        rows, cpad = self._cv(self.fwd, f"{k}.conv2", a1, [(z2, Cout, 0, 0, Cout, 0)], f"{k}.conv2.weight", Ho, Wo, Ho, Wo, 3, 1, 1, Cout, Cout,
                              stats=self.training)
        rows2, cpad2 = rows, cpad
        # bn2: its statistics finish inside the apply pass below when that is available (bnfused.hip: one launch instead of two; the
        # downsample branch in between writes other rows of the shared statistics scratch, so it needs its own finalize first)
        down = f"{k}.downsample.0.weight" in self.m._pspec
        fuse2 = (self.training and not down and self._bn_fused
                 and bool(self.lib.ksmi_bn_fused_supported(Cout, cpad2, dt)))
        if not fuse2:
            self._bn_finalize(f"{k}.bn2", sv2, rows, cpad, Cout, npix)
        if down:
            ds, idn = self.buf(B, Ho, Wo, Cout), self.buf(B, Ho, Wo, Cout)
            svd = _Saved(Cout, self.dev)
            rows, cpad = self._cv(self.fwd, f"{k}.downsample", [SrcSpec(x_in, Cin)], [(ds, Cout, 0, 0, Cout, 0)], f"{k}.downsample.0.weight", H, W, Ho, Wo,
                                  1, stride, 0, Cout, Cin, stats=self.training)
            self._bn_finalize(f"{k}.downsample.1", svd, rows, cpad, Cout, npix)
            self._affine(self.fwd, ds, svd, idn, npix, Cout, 0)
        else:
            idn = x_in
        if fuse2:
            m = self.m
            kb = f"{k}.bn2"
            g2, b2 = m._p(f"{kb}.weight").data_ptr(), m._p(f"{kb}.bias").data_ptr()
            rm, rv, nbt = m._b(f"{kb}.running_mean").data_ptr(), m._b(f"{kb}.running_var").data_ptr(), m._c(f"{kb}.num_batches_tracked").data_ptr()
            st = self._stats_ptr()
            self.fwd.add("ksmi_bn_fin_add_relu", lambda: (st(), rows2, cpad2, Cout, float(npix), g2, b2, rm, rv, nbt, BN_MOMENTUM, BN_EPS,
                                                          sv2.mean, sv2.rstd, sv2.scale, sv2.shift, z2.data_ptr(), idn.data_ptr(), out.data_ptr(),
                                                          None, B, Ho, Wo, dt), self._elt_meta("bn_add_relu", 3 * npix * Cout))
        else:
            self.fwd.add("ksmi_bn_add_relu", lambda: (z2.data_ptr(), idn.data_ptr(), sv2.scale, sv2.shift, out.data_ptr(), npix, Cout, dt),
                         self._elt_meta("bn_add_relu", 3 * npix * Cout))

        def bwd():
            dout = self.gbuf(out)
            dz2, da1, di1 = self.buf(B, Ho, Wo, Cout), self.buf(B, Ho, Wo, Cout), self.buf(B, Ho, Wo, Cout)
            self._bnrelu_bwd(f"{k}.bn2", dout, out, z2, sv2, dz2, npix, Cout)            # dout now holds g = dout * (out > 0)
            # conv2
            self._wg(a1, dz2, Cout, f"{k}.conv2.weight", Ho, Wo, Ho, Wo, 3, 1, 1, Cout)
            r2, c2 = self._conv3(self.bwd, f"{k}.conv2", [SrcSpec(dz2, Cout)], [(da1, Cout, 0, 0, Cout, 0)], f"{k}.conv2.weight", None, B, Ho, Wo, Cout, Cout,
                                 mask=self._bnmask(i1, sv1), stats=True, dgrad=True)
            self._bn_backward(f"{k}.bn1", da1, i1, sv1, di1, r2, c2, Cout, npix, npix, 0)
            # conv1
            self._wg([SrcSpec(x_in, Cin)], di1, Cout, f"{k}.conv1.weight", H, W, Ho, Wo, 3, stride, 1, Cin)
            dx = self.gbuf(x_in)
            acc = self.gacc(x_in)
            if stride == 1:
                self._conv3(self.bwd, f"{k}.conv1", [SrcSpec(di1, Cout)], [(dx, Cin, 0, 0, Cin, acc)], f"{k}.conv1.weight", None, B, H, W, Cin, Cout, dgrad=True)
            else:
                self._dgrad_s2(f"{k}.conv1", di1, Cout, dx, Cin, H, W, f"{k}.conv1.weight", acc)
            # identity branch
            if down:
                dds = self.buf(B, Ho, Wo, Cout)
                self._bn_plain_bwd(f"{k}.downsample.1", dout, ds, svd, dds, npix, Cout)
                self._wg([SrcSpec(x_in, Cin)], dds, Cout, f"{k}.downsample.0.weight", H, W, Ho, Wo, 1, stride, 0, Cin)
                d, table = make_conv([SrcSpec(dds, Cout)], [(dx, Cin, 0, 0, Cin, 1)], dx, None, None, B, Ho, Wo, Ho, Wo, 1, 1, 1, 0, Cin, self.dtype,
                                     out_map=(stride, stride, 0, 0, H, W) if stride != 1 else None)   # (stride 1: BIT-CD's layer3 / layer4)
                d.wpk = self._packed(f"{k}.downsample.0.weight", table, 1, Cin, Cin, Cin, 1, 0, 0).data_ptr()
                self._conv(self.bwd, d, "dgrad_1x1s2", f"{k}.downsample")
            else:
                self.bwd.add("ksmi_add", lambda: (dx.data_ptr(), dout.data_ptr(), dx.data_ptr(), npix * Cout, dt), self._elt_meta("add", 3 * npix * Cout))
        self._bwd.append(bwd)
        return out


class UnetPlan(ResNetPlan):
    def __init__(self, model, B, H, W, dtype, training, with_backward):
        self._init_conv(model, B, H, W, dtype, training, with_backward)
        self.cin, self.nc = model.in_channels, model.classes
        self.x = torch.empty((B, self.cin, H, W), dtype=torch.float32, device=self.dev)
        self.logits = torch.empty((B, self.nc, H, W), dtype=torch.float32, device=self.dev)
        self.dlogits = torch.empty_like(self.logits) if with_backward else None
        self._build_lists(self._build_unet)

    # ---------------------------------------------------------------- DecoderBlock (smp unet/decoder.py)
    def _decoder_block(self, k, xd, Cin, skips, Cout, h, w, U=None, up_out=False, multi_writer=False):
        """y = conv3x3-BN-ReLU twice over cat(nearest x2 of xd, *skips); skips = [(tensor, channels), ...] at 2h x 2w, in concat order.
        U: the upsampled xd when its producer already wrote it (up_out of that block).  up_out: y feeds a next block as its upsampled
        input, so the BatchNorm apply also writes the x2 copy (self._up[id(y)], ksmi_affine_relu_upsample2).  multi_writer: d(xd) may
        have earlier writers (UNet++: xd is also somebody's skip), so its upsample backward takes the accumulate flag."""
        B, dt = self.B, self.dt
        H2, W2 = 2 * h, 2 * w
        npix = B * H2 * W2
        if U is None:
            U = self.buf(B, H2, W2, Cin)
            self.fwd.add("ksmi_upsample2_forward", lambda: (xd.data_ptr(), U.data_ptr(), B, h, w, Cin, 0, dt), self._elt_meta("upsample2", 5 * B * h * w * Cin))
        z1, z2, y = self.buf(B, H2, W2, Cout), self.buf(B, H2, W2, Cout), self.buf(B, H2, W2, Cout)
        svA, svB = _Saved(max(Cout, 16), self.dev), _Saved(max(Cout, 16), self.dev)
        srcs = [SrcSpec(U, Cin)] + [SrcSpec(t, cs) for t, cs in skips]
        Kt = Cin + sum(cs for _, cs in skips)
        rows, cpad = self._cv(self.fwd, f"{k}.conv1", srcs, [(z1, Cout, 0, 0, Cout, 0)], f"{k}.conv1.0.weight", H2, W2, H2, W2, 3, 1, 1, Cout, Kt, stats=self.training)
        self._bn_finalize(f"{k}.conv1.1", svA, rows, cpad, Cout, npix)
        a1 = [SrcSpec(z1, Cout, scale=svA.scale_t, shift=svA.shift_t, relu=1)]
        rows, cpad = self._cv(self.fwd, f"{k}.conv2", a1, [(z2, Cout, 0, 0, Cout, 0)], f"{k}.conv2.0.weight", H2, W2, H2, W2, 3, 1, 1, Cout, Cout, stats=self.training)
        self._bn_finalize(f"{k}.conv2.1", svB, rows, cpad, Cout, npix)
        if up_out:
            Uy = self._up[id(y)] = self.buf(B, 2 * H2, 2 * W2, Cout)
            self.fwd.add("ksmi_affine_relu_upsample2", lambda: (z2.data_ptr(), svB.scale, svB.shift, y.data_ptr(), Uy.data_ptr(), B, H2, W2, Cout, dt),
                         self._elt_meta("bn_apply_up2", 6 * npix * Cout))
        else:
            self._affine(self.fwd, z2, svB, y, npix, Cout, 1)

        def bwd():
            dy = self.gbuf(y)
            dz2, da1, dz1, dU = self.buf(B, H2, W2, Cout), self.buf(B, H2, W2, Cout), self.buf(B, H2, W2, Cout), self.buf(B, H2, W2, Cin)
            self._bnrelu_bwd(f"{k}.conv2.1", dy, y, z2, svB, dz2, npix, Cout)
            self._wg(a1, dz2, Cout, f"{k}.conv2.0.weight", H2, W2, H2, W2, 3, 1, 1, Cout)
            r2, c2 = self._conv3(self.bwd, f"{k}.conv2", [SrcSpec(dz2, Cout)], [(da1, Cout, 0, 0, Cout, 0)], f"{k}.conv2.0.weight", None, B, H2, W2, Cout, Cout,
                                 mask=self._bnmask(z1, svA), stats=True, dgrad=True)
            self._bn_backward(f"{k}.conv1.1", da1, z1, svA, dz1, r2, c2, Cout, npix, npix, 0)
            self._wg(srcs, dz1, Cout, f"{k}.conv1.0.weight", H2, W2, H2, W2, 3, 1, 1, Kt)
            dsts, off = [(dU, Cin, 0, 0, Cin, 0)], Cin
            for t, cs in skips:
                dsts.append((self.gbuf(t), cs, 0, off, cs, self.gacc(t)))
                off += cs
            self._conv3(self.bwd, f"{k}.conv1", [SrcSpec(dz1, Cout)], dsts, f"{k}.conv1.0.weight", None, B, H2, W2, Kt, Cout, dgrad=True)
            dxd = self.gbuf(xd)
            acc = self.gacc(xd)
            if multi_writer:
                self.bwd.add("ksmi_upsample2_backward_acc", lambda: (dU.data_ptr(), None, dxd.data_ptr(), acc, B, h, w, Cin, 0, dt),
                             self._elt_meta("upsample2_bwd", (5 + acc) * B * h * w * Cin))
                return
            if acc:
                raise _lib.KsmiError("unexpected second writer of a decoder input gradient")
            self.bwd.add("ksmi_upsample2_backward", lambda: (dU.data_ptr(), None, dxd.data_ptr(), B, h, w, Cin, 0, dt), self._elt_meta("upsample2_bwd", 5 * B * h * w * Cin))
        self._bwd.append(bwd)
        return y

    # ---------------------------------------------------------------- the graph
    def _build_encoder(self):
        """stem and layer1..4 -> ([f1..f5], height, width of f5)"""
        f1, p, H2, W2 = self._resnet_stem("encoder", self.x)
        feats = [f1]
        t, cin, h, w = p, 64, H2, W2
        for li, (ch, stride) in enumerate(LAYERS):
            for bi in range(2):
                s_ = stride if bi == 0 else 1
                t = self._basic_block(f"encoder.layer{li + 1}.{bi}", t, cin, ch, h, w, s_)
                h, w, cin = h // s_, w // s_, ch
            feats.append(t)
        self.named.update({f"f{i + 1}": f for i, f in enumerate(feats)})
        return feats, h, w

    def _build_head(self, y):
        """segmentation head: conv3x3(16 -> classes) + bias on the last decoder output"""
        B, H, W, dt = self.B, self.H, self.W, self.dt
        P = self.buf(B, H, W, CS)
        nc = self.nc
        self._cv(self.fwd, "segmentation_head", [SrcSpec(y, 16)], [(P, CS, 0, 0, nc, 0)], "segmentation_head.0.weight", H, W, H, W, 3, 1, 1, nc, 16,
                 bkey="segmentation_head.0.bias")
        HW = H * W
        self.fwd.add("ksmi_out_to_nchw", lambda: (P.data_ptr(), self.logits.data_ptr(), B, nc, CS, HW, 0, dt))
        self._bwd.append(lambda: self._class_head_bwd("segmentation_head", "segmentation_head.0.weight", "segmentation_head.0.bias", y, 16))

    def _build_unet(self):
        feats, h, w = self._build_encoder()
        skips = feats[::-1]                      # f5, f4, f3, f2, f1
        chans = (512, 256, 128, 64, 64)
        y, cy = skips[0], 512
        for i, co in enumerate(DECODER_CHANNELS):
            skip = [(skips[i + 1], chans[i + 1])] if i + 1 < len(skips) else []
            y = self._decoder_block(f"decoder.blocks.{i}", y, cy, skip, co, h, w)
            self.named[f"d{i}"] = y
            h, w, cy = 2 * h, 2 * w, co
        self._build_head(y)

    # ---------------------------------------------------------------- execution
    def run_forward(self, x):
        return self._run_forward(self.logits, (x, self.x))


class UnetPlusPlusPlan(UnetPlan):
    """smp UnetPlusPlusDecoder on the same pieces (unetpp.py: the block table and the forward order): eleven DecoderBlocks on a dense grid.
    Every feature map has several gradient writers ("=" by the first, "+=" by the later ones, through gacc): the blocks are built in
    forward order, so the reversed closure list runs every consumer of a tensor before its producer.  A block output that is the next
    block's upsampled input gets its x2 copy from the BatchNorm apply pass (KSMI_UNETPP_FUSED_UP=0: the two-launch pair, for the A/B)."""

    def _build_unet(self):
        from .unetpp import block_table, forward_order
        fused = os.environ.get("KSMI_UNETPP_FUSED_UP", "1") != "0"
        self._up = {}
        feats, h5, w5 = self._build_encoder()
        features = feats[::-1]                   # f5, f4, f3, f2, f1
        table, x = block_table(), {}
        for name in forward_order():
            d, l = (int(v) for v in name.split("_")[1:])
            ci, cs, co = table[name]
            xd = features[d] if l == d else x[(d, l - 1)]
            skips = [(x[(i, l)], table[f"x_{i}_{l}"][2]) for i in range(d + 1, l + 1)] if l < 4 else []
            if l < 4:
                skips.append((features[l + 1], cs // (l + 1 - d)))
            assert ci == xd.shape[-1] and cs == sum(c for _, c in skips) and all(t.shape[-1] == c for t, c in skips), name
            up_out = fused and (l < 3 or name == "x_0_3")        # x_d_l is the upsampled input of x_d_{l+1}
            y = self._decoder_block(f"decoder.blocks.{name}", xd, ci, skips, co, h5 << l, w5 << l, U=self._up.get(id(xd)), up_out=up_out,
                                    multi_writer=True)
            x[(d, l)] = self.named[name] = y
        self._build_head(x[(0, 4)])
