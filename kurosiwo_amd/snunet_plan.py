"""Static launch plan of one SNUNet-ECAM forward/backward at a fixed (B, H, W, dtype, mode).

The plan owns every NHWC activation / gradient buffer and a flat list of prepared C-ABI
calls; running it is a loop of ctypes calls on the current HIP stream (no allocation, no
host sync), so a whole train step can be captured into one HIP graph.

Reference computation: /root/reference/models/snunet.py:118-153 (forward graph),
:11-29 (conv_block_nested), :32-46 (up), :49-62 + :146-151 (ECAM head).
"""
import ctypes as C
import os

import torch

from . import _lib
from .plan_base import PlanBase, _Saved
from .runtime import Act, SrcSpec, conv_npad, conv_stats_rows, make_conv, make_pack, make_wgrad, packed_weight_numel
from .snunet import BN_EPS, BN_MOMENTUM


class SNUNetPlan(PlanBase):
    side_wgrad = True          # weight gradients on the train step's side stream (see LaunchList.run; plan_base.PlanBase.side_wgrad)
    two_lanes = True           # the decoder launches carry lane tags and hand-over entries (StepStreams)
    bn_fused = os.environ.get("KSMI_BN_FUSED", "1") != "0"     # statistics finish inside the consuming pass (csrc/bnfused.hip)
    im2col_late = os.environ.get("KSMI_IM2COL_LATE", "1") != "0"   # first-layer im2col in the backward list, next to its reader
    up_gemm = os.environ.get("KSMI_UP_GEMM", "1") != "0"           # ConvTranspose2d(k2, s2) with C >= 128 as token GEMMs (ksmi_up_*)
    up_wgrad64 = os.environ.get("KSMI_UP_WGRAD64", "1") != "0"     # ... and the level-0 Up weight gradients (C = 64)
    up_wgrad128 = os.environ.get("KSMI_UP_WGRAD128", "1") != "0"   # ... and the level-1 ones (C = 128; after the reducer was parallelised)
    pack_kind = "pack_weights_batched"

    def __init__(self, model, B, H, W, dtype, training, with_backward, tail=0, sync_bn=False):
        self._init_lists(model, dtype, with_backward)        # (no bf16 parameter mirror: the convolutions read packed weights)
        self.B, self.H, self.W = B, H, W
        # SyncBN (optional, SURVEY.md §8(e) "second-order items"): BatchNorm statistics of the GLOBAL batch -- the statistics rows of every
        # BatchNorm call (forward: sum, sum of squares; backward: sum g, sum g * xhat) are summed over the ranks before they are
        # finished, with the global pixel count.  Data parallelism with it equals one process on the whole batch
        # (tests/test_gpu_dp.py::test_syncbn_two_ranks_equal_single_process); the default (off) is the reference's per-rank BatchNorm
        # (models/snunet.py:16,18 under DataParallel-free training).  Uses the unfused statistics passes (one tiny collective per call).
        from . import distributed as _D
        self.sync_bn = bool(sync_bn) and training
        self.bn_world = _D.world_size() if self.sync_bn else 1
        if self.sync_bn:
            self.bn_fused = False
        self.training = training
        self._up_packs = []        # (ConvTranspose weight, its [4C][C] bf16 image, C) of the `up` layers on the token-GEMM path
        # deferred row reductions (bias gradients): (RowsumDesc, parameter key) -> ONE launch ending the backward (PlanBase's batches of
        # `rowsum_batch`, _rs_entries, stay empty here)
        self._rowsums = []
        n, c = model.base_channel, model.in_channels
        self.n = n
        f = [n, 2 * n, 4 * n, 8 * n, 16 * n]
        # `tail` trailing input channels (the DEM) are shared by both dates and live in their own buffer: the first conv reads
        # channels [0, c - tail) from xA / xB and the rest from xtail (the trainer's torch.cat((image, dem), 1) as an address choice)
        self.tail = tail
        self.xA = torch.empty((B, c - tail, H, W), dtype=torch.float32, device=self.dev)
        self.xB = torch.empty_like(self.xA)
        self.xtail = torch.empty((B, tail, H, W), dtype=torch.float32, device=self.dev) if tail else None
        self.logits = torch.empty((B, 3, H, W), dtype=torch.float32, device=self.dev)
        self.dlogits = torch.empty_like(self.logits) if with_backward else None
        self.bwd_builders = []

        def A(name, lvl, ch):
            return Act(name, B, H >> lvl, W >> lvl, ch, dtype, self.dev)

        # ---- forward graph (snunet.py:118-153) -----------------------------------------------
        # Siamese encoder, level by level: date A on lane 0, date B on lane 1, B one block behind A.  Both dates share every parameter:
        # BatchNorm running statistics are updated A first, then B (the reference's order, snunet.py:121-130), and in the backward list
        # (built in reverse) the date-B block writes the shared BatchNorm gradients ("=") before the date-A block accumulates ("+=");
        # the hand-over entries between the two blocks of a level keep exactly that order on two streams.
        L = self._lane
        L(0); x0_0A, p0A = self._block("conv0_0", "A", [self.xA], A("x0_0A", 0, f[0]), first=True, pool="p0A")
        self._handover(0, 1, back=(1, 0))
        L(1); x0_0B, p0B = self._block("conv0_0", "B", [self.xB], A("x0_0B", 0, f[0]), first=True, pool="p0B")
        L(0); x1_0A, p1A = self._block("conv1_0", "A", [self._pool_at(x0_0A, p0A, "p0A")], A("x1_0A", 1, f[1]), pool="p1A")
        self._handover(0, 1, back=(1, 0))
        L(1); x1_0B, p1B = self._block("conv1_0", "B", [self._pool_at(x0_0B, p0B, "p0B")], A("x1_0B", 1, f[1]), pool="p1B")
        L(0); x2_0A, p2A = self._block("conv2_0", "A", [self._pool_at(x1_0A, p1A, "p1A")], A("x2_0A", 2, f[2]), pool="p2A")
        self._handover(0, 1, back=(1, 0))
        L(1); x2_0B, p2B = self._block("conv2_0", "B", [self._pool_at(x1_0B, p1B, "p1B")], A("x2_0B", 2, f[2]), pool="p2B")
        L(0); x3_0A = self._block("conv3_0", "A", [self._pool_at(x2_0A, p2A, "p2A")], A("x3_0A", 3, f[3]))
        self._handover(0, 1, back=(1, 0))
        L(1); x3_0B, p3B = self._block("conv3_0", "B", [self._pool_at(x2_0B, p2B, "p2B")], A("x3_0B", 3, f[3]), pool="p3B")
        x4_0B = self._block("conv4_0", "B", [self._pool_at(x3_0B, p3B, "p3B")], A("x4_0B", 4, f[4]))
        self._handover(1, 0, back=(0, 1))                  # encoder | decoder: both lanes have everything of the other side

        # Decoder on two lanes (LaunchList.run / StepStreams): lane 0 = the level-0 column blocks + the head, lane 1 = every deeper block and the Ups
        # leaving it (Up1_0, fed by the encoder, stays with lane 0).  Lane 1 needs the encoder only; lane 0 needs lane 1 through
        # x1_j -> Up1_j (forward) and lane 1 needs lane 0 through d Up1_j -> d x1_j (backward): three ordered hand-overs each way.
        # The level-0 blocks carry the large BatchNorm / elementwise passes (224^2 maps), the deeper blocks are convolution-bound.
        self._handover(0, 1, back=(1, 0))
        L(0); x0_1 = self._block("conv0_1", "", [x0_0A, x0_0B, self._up("Up1_0", x1_0B)], A("x0_1", 0, f[0]))
        L(1); x1_1 = self._block("conv1_1", "", [x1_0A, x1_0B, self._up("Up2_0", x2_0B)], A("x1_1", 1, f[1]))
        u1_1 = self._up("Up1_1", x1_1)                      # (the Up1_j ride on lane 1 with their source block: lane 0 is the longer one)
        self._handover(1, 0, back=(0, 1))
        L(0); x0_2 = self._block("conv0_2", "", [x0_0A, x0_0B, x0_1, u1_1], A("x0_2", 0, f[0]))
        L(1); x2_1 = self._block("conv2_1", "", [x2_0A, x2_0B, self._up("Up3_0", x3_0B)], A("x2_1", 2, f[2]))
        x1_2 = self._block("conv1_2", "", [x1_0A, x1_0B, x1_1, self._up("Up2_1", x2_1)], A("x1_2", 1, f[1]))
        u1_2 = self._up("Up1_2", x1_2)
        self._handover(1, 0, back=(0, 1))
        L(0); x0_3 = self._block("conv0_3", "", [x0_0A, x0_0B, x0_1, x0_2, u1_2], A("x0_3", 0, f[0]))
        L(1); x3_1 = self._block("conv3_1", "", [x3_0A, x3_0B, self._up("Up4_0", x4_0B)], A("x3_1", 3, f[3]))
        x2_2 = self._block("conv2_2", "", [x2_0A, x2_0B, x2_1, self._up("Up3_1", x3_1)], A("x2_2", 2, f[2]))
        x1_3 = self._block("conv1_3", "", [x1_0A, x1_0B, x1_1, x1_2, self._up("Up2_2", x2_2)], A("x1_3", 1, f[1]))
        u1_3 = self._up("Up1_3", x1_3)
        self._handover(1, 0, back=(0, 1))
        L(0); x0_4 = self._block("conv0_4", "", [x0_0A, x0_0B, x0_1, x0_2, x0_3, u1_3], A("x0_4", 0, f[0]))
        self._head([x0_1, x0_2, x0_3, x0_4])
        self.acts = {a.name: a for a in (x0_0A, x0_0B, x1_0A, x1_0B, x3_0B, x4_0B, x0_1, x1_1, x0_2, x0_3, x0_4, x1_3, x3_1)}

        if with_backward:
            for lane, build in reversed(self.bwd_builders):
                self._lane(lane)
                build()
            self._lane(0)
        self._finish()

    def _before_pack_table(self):
        """the one row-sum launch that ends the backward list, and the weight images of the token-GEMM `up` layers"""
        if self._rowsums:
            nr = len(self._rowsums)
            arr_r = (_lib.RowsumDesc * nr)(*[r for r, _ in self._rowsums])
            raw_r = bytes(C.string_at(C.addressof(arr_r), C.sizeof(arr_r)))
            rtable = torch.frombuffer(bytearray(raw_r), dtype=torch.uint8).to(self.dev)
            self.keep.append(rtable)
            self.bwd.add("ksmi_reduce_rows_batched", lambda: (rtable.data_ptr(), nr))
            self._mark(*[k for _, k in self._rowsums])
        for i in range(0, len(self._up_packs), 16):           # KSMI_UP_PACK_MAX tensors per launch
            grp = self._up_packs[i:i + 16]
            wt_a = (C.c_void_p * len(grp))(*[w.data_ptr() for w, _, _ in grp])
            wb_a = (C.c_void_p * len(grp))(*[b.data_ptr() for _, b, _ in grp])
            c_a = (C.c_int * len(grp))(*[c for _, _, c in grp])
            self.keep += [wt_a, wb_a, c_a]
            self.packs.add("ksmi_up_pack_weights_batched", lambda wt_a=wt_a, wb_a=wb_a, c_a=c_a, k=len(grp): (wt_a, wb_a, c_a, k),
                           {"kind": "up_pack_weight", "bytes": sum(4 * c * c * 6 for _, _, c in grp), "flops": 0})

    # ---------------------------------------------------------------- helpers
    def _lane(self, lane):
        """launches appended from here on belong to compute lane `lane`"""
        self.fwd.cur_lane = self.bwd.cur_lane = lane

    def _level(self, H):
        """measurement tag: the resolution level of the maps a module works on (L0 = full resolution ... L4 = 1/16)"""
        lvl = {self.H >> k: k for k in range(5)}.get(H)
        self._stage(None if lvl is None else f"L{lvl}")

    def _sname(self, name):
        """scratch buffers that live from one launch to the next of the same block are per lane"""
        return name if self.fwd.cur_lane == 0 else f"{name}@{self.fwd.cur_lane}"

    def _handover(self, src, dst, back):
        """forward list: lane dst continues behind everything lane src was handed so far; backward list (built in reverse): lane
        back[1] behind lane back[0] at the mirrored position"""
        self.fwd.add_wait(src, dst)
        a, b = back
        self.bwd_builders.append((0, lambda: self.bwd.add_wait(a, b)))

    def _rows(self, npix):
        return max(1, min(512, npix // 256))

    def _rowsum_at_end(self, key, partial, rows, K, k, Cstride, Cc):
        """grad[key][c] (+)= sum_rows partial[(r*K + k)*Cstride + c] in the batched launch that ends the backward; partial = None: zeros"""
        r = _lib.RowsumDesc()
        r.partial = partial.data_ptr() if partial is not None else None
        r.dst = self.m._g(key).data_ptr()
        r.rows, r.K, r.k, r.Cstride, r.C = (rows if partial is not None else 0), K, k, Cstride, Cc
        r.accumulate, r.head, r.next = 0, 1, -1
        if self._acc_param(key):                      # a second call of the same module (siamese branches): chain behind the first entry
            prev = [q for q, kk in self._rowsums if kk == key][-1]
            prev.next, r.head = len(self._rowsums), 0
        if partial is not None:
            self.keep.append(partial)
        self._rowsums.append((r, key))

    def _conv(self, ll, d, tag="fwd", name=""):
        self.keep.append(d)
        meta, ktot, _ = self._conv_meta(d, tag, f",BN{32 if d.Npad >= 32 else 16}")
        meta["tag"] = f"K={ktot} N={d.N} {d.Hout}x{d.Wout} nsrc={d.nsrc}"
        ll.add("ksmi_conv_forward", lambda: (C.byref(d), self.dt), meta)

    def _side_ix(self, key):
        """side stream of a parameter's weight gradient (KSMI_SIDE2=1: alternating by first appearance; a parameter keeps its stream, so
        the two launches of a shared encoder weight stay ordered)"""
        if os.environ.get("KSMI_SIDE2", "0") != "1":
            return 0
        if not hasattr(self, "_side_of"):
            self._side_of = {}
        if key not in self._side_of:
            self._side_of[key] = len(self._side_of) & 1
        return self._side_of[key]

    def _wgrad(self, d, ws, key, side_tag=None):
        assert side_tag is None              # (tagged waits are the token plans' scheme: nothing here overwrites a weight gradient's operands)
        self.keep.append(d)
        # the partial-slab scratch is per compute lane: with the side stream off (or a timed launch) the weight gradients of the two
        # lanes run concurrently on their lanes' streams (and per side stream: two weight gradients in flight own two slabs)
        six = self._side_ix(key)
        sW = self._sname("wgrad" + ("_s2" if six else ""))
        self.need(sW, ws)
        self.patch(d, "partial", sW)
        meta, ktot, _ = self._wgrad_meta(d)
        meta["tag"] = f"{key} K={ktot} N={d.N} {d.Hout}x{d.Wout}"
        meta["side"] = True                  # off the critical path: eligible for the side stream (LaunchList.run)
        meta["side_ix"] = six
        self.bwd.add("ksmi_conv_wgrad", lambda: (C.byref(d), self.dt), meta)
        self._mark(key)

    # ---------------------------------------------------------------- "virtual sum" input gradient
    def _emit_dgrad(self, act, bias_key=None, gate=None):
        """d act = sum over the 3x3 convs that read `act` of convT(di_j, W_j[:, slice_j]) as ONE implicit GEMM
        whose K axis walks the consumers' `di` tensors (the dual of the forward's virtual concat): every
        gradient tensor is written once instead of read-modify-written per consumer, and K grows from
        Cout_j to sum_j Cout_j.  Consumers registered themselves in their own build_bwd (earlier in the
        backward order)."""
        cons = getattr(act, "consumers", [])
        if not cons:
            return False
        B, H, W, Cc = act.B, act.H, act.W, act.C
        srcs = [SrcSpec(r, cj) for (r, cj, _, _, _) in cons]
        acc = act.take_acc_flag()
        d, table = make_conv(srcs, [(act.grad(), Cc, 0, 0, Cc, acc)], act.grad(), None, None, B, H, W, H, W, 3, 3, 1, 1, Cc, self.dtype)
        Npad = conv_npad(Cc)
        wpk = torch.empty(packed_weight_numel(table, 9, Npad, self.dtype), dtype=self.dtype, device=self.dev)
        kc = 32 if self.dtype == torch.bfloat16 else 16
        slab = 9 * Npad * kc
        ch0 = 0
        for (r, cj, wkey, coff, ktot) in cons:
            nch = -(-cj // kc)
            tj = [(0, c0, c0, min(kc, cj - c0)) for c0 in range(0, cj, kc)]
            # element (chunk, tap', col = c_local, kk = n_local) = W_j[n][coff + c_local][flip(tap')]
            wview = self.m._p(wkey)[coff * 9:]
            out = wpk[ch0 * slab:(ch0 + nch) * slab]
            pd = make_pack(wview, out, tj, 9, Cc, Npad, Cc, ktot * 9, 9, 0, 1, 1)
            self.keep += [pd, wview, out]
            self._pack_descs.append(pd)
            ch0 += nch
        d.wpk = wpk.data_ptr()
        self.keep.append(wpk)
        gated = None
        if gate is not None:
            g_out, g_z, g_sv = gate
            d.gate_src, d.xhat_src, d.g_mean, d.g_rstd = g_out.data_ptr(), g_z.data_ptr(), g_sv.mean, g_sv.rstd
            if self.lib.ksmi_conv_gate_supported(C.byref(d), self.dt):
                rows_g = conv_stats_rows(d, self.dtype)
                st = torch.empty(rows_g * 2 * Npad, dtype=torch.float32, device=self.dev)
                d.stats = st.data_ptr()
                self.keep.append(st)
                gated = (st, rows_g, Npad)
            else:
                d.gate_src = d.xhat_src = d.g_mean = d.g_rstd = None
        if bias_key is not None:
            # `act` is the output of a ConvTranspose2d whose bias gradient is sum_pixels d act: the statistics epilogue of this launch
            # emits the per-tile sums (was: one more pass over the gradient tensor, ksmi_channel_sum)
            rows_g = conv_stats_rows(d, self.dtype)
            st = torch.empty(rows_g * 2 * Npad, dtype=torch.float32, device=self.dev)
            d.stats = st.data_ptr()
            self._rowsum_at_end(bias_key, st, rows_g, 2, 0, Npad, Cc)
        self._conv(self.bwd, d, "dgrad")
        return gated if gated is not None else True

    # ---------------------------------------------------------------- nn.MaxPool2d(2,2)  (snunet.py:73)
    def _pool(self, x, name):
        y = Act(name, x.B, x.H // 2, x.W // 2, x.C, self.dtype, self.dev)
        self._level(x.H)
        self.fwd.add("ksmi_maxpool2x2_forward", lambda: (x.t.data_ptr(), y.t.data_ptr(), x.B, x.H, x.W, x.C, self.dt))
        self._pool_bwd(x, y)
        return y

    def _pool_at(self, x, y, name):
        """the pooled copy of an encoder block output at this point of the lists: y from the fused block tail (only its backward is
        registered here, at the place the stand-alone pool has in the launch order), or None -> the stand-alone launch"""
        if y is None:
            return self._pool(x, name)
        self._pool_bwd(x, y)
        return y

    def _pool_bwd(self, x, y):
        """backward of y = maxpool2x2(x) (y written by ksmi_maxpool2x2_forward or by the fused block tail)"""
        def build_bwd():
            self._level(x.H)
            self._emit_dgrad(y)
            acc = x.take_acc_flag()
            gy, gx = y.grad(), x.grad()
            self.bwd.add("ksmi_maxpool2x2_backward", lambda: (x.t.data_ptr(), gy.data_ptr(), gx.data_ptr(), acc,
                                                              x.B, x.H, x.W, x.C, self.dt))
        self.bwd_builders.append((self.fwd.cur_lane, build_bwd))

    def _up_conv_forward(self, x, y, wkey, bkey, B, H, W, Cc):
        d, table = make_conv([SrcSpec(x.t, Cc)], [(y.t, Cc, 0, 0, 4 * Cc, 0)], x.t, self.m._p(bkey), None,
                             B, H, W, H, W, 1, 1, 1, 0, 4 * Cc, self.dtype, ps_cout=Cc)
        # Wt[c][n][dy][dx]: GEMM column j = d*C + n, k = c
        wpk = self._packed(wkey, table, 1, 4 * Cc, Cc, Cc * 4, 4, 1, 0, 0)
        d.wpk = wpk.data_ptr()
        self._conv(self.fwd, d)

    # ---------------------------------------------------------------- up = ConvTranspose2d(k2,s2)  (snunet.py:32-46)
    def _up(self, name, x):
        Cc, B, H, W = x.C, x.B, x.H, x.W
        y = Act(name, B, 2 * H, 2 * W, Cc, self.dtype, self.dev)
        self._level(2 * H)                                   # (an Up is booked on the level it writes)
        wkey, bkey = f"{name}.up.weight", f"{name}.up.bias"
        # levels with C >= 128 (Up2_j, Up3_j, Up4_0): the transposed convolution and both of its gradients as token GEMMs over the
        # "depth rows" of the output (csrc/gemm2.hip, ksmi_up_*): 400-600 TFLOP/s kernels instead of the 140-240 TFLOP/s the k2 s2
        # shapes reach on the first-generation convolution kernels
        up_gemm = (self.up_gemm and self.dtype == torch.bfloat16 and bool(self.lib.ksmi_up_gemm_supported(B, H, W, Cc, self.dt)))
        # measured per operation (profiles/r04_up_gemm.txt, one stream): the input gradient (K = 4C) wins from C = 128 on (76 -> 49 us at
        # 56^2), forward and weight gradient from C = 256 on (77 -> 57 us, 79 -> ~40 us at 28^2); at C = 128 the forward GEMM has two K
        # steps per tile and loses to the persistent 1x1 kernel (33-45 -> 80 us), the weight gradient ties (73 -> 70 us)
        up_fwd_gemm = up_gemm and Cc >= 256
        up_wgrad_gemm = up_fwd_gemm or (self.up_gemm and ((self.up_wgrad64 and Cc == 64) or (self.up_wgrad128 and Cc == 128))
                                        and self.dtype == torch.bfloat16 and bool(self.lib.ksmi_up_wgrad_supported(B, H, W, Cc, self.dt)))
        es = self._es()
        if up_gemm:
            wb = torch.empty(4 * Cc * Cc, dtype=torch.bfloat16, device=self.dev)
            self.keep.append(wb)
            self._up_packs.append((self.m._p(wkey), wb, Cc))        # one batched launch for all of them (end of __init__)
        if up_fwd_gemm:
            self.fwd.add("ksmi_up_forward", lambda: (x.t.data_ptr(), wb.data_ptr(), self.m._p(bkey).data_ptr(), y.t.data_ptr(), B, H, W, Cc),
                         {"kind": "up_gemm_fwd", "bytes": B * H * W * Cc * 5 * es, "flops": 2 * B * H * W * Cc * 4 * Cc, "tag": f"K={Cc} N={4 * Cc} {H}x{W}"})
        else:
            self._up_conv_forward(x, y, wkey, bkey, B, H, W, Cc)

        def build_bwd():
            self._level(2 * H)
            fused_bias = self._emit_dgrad(y, bias_key=bkey)
            gy = y.grad()
            s2 = [SrcSpec(gy, Cc)]
            acc = x.take_acc_flag()
            if up_gemm:
                gx = x.grad()
                self.bwd.add("ksmi_up_dgrad", lambda: (gy.data_ptr(), wb.data_ptr(), gx.data_ptr(), acc, B, H, W, Cc),
                             {"kind": "up_gemm_dgrad", "bytes": B * H * W * Cc * (5 + acc) * es, "flops": 2 * B * H * W * Cc * 4 * Cc,
                              "tag": f"K={4 * Cc} N={Cc} {H}x{W}"})
            else:
                # input gradient = 2x2 stride-2 conv over dUp: K = n, N = c
                d2, t2 = make_conv(s2, [(x.grad(), Cc, 0, 0, Cc, acc)], gy, None, None,
                                   B, 2 * H, 2 * W, H, W, 2, 2, 2, 0, Cc, self.dtype)
                w2 = self._packed(wkey, t2, 4, Cc, Cc, 4, Cc * 4, 0, 1, 0)
                d2.wpk = w2.data_ptr()
                self._conv(self.bwd, d2, "dgrad")
            if up_wgrad_gemm:
                six = self._side_ix(wkey)
                sW = self._sname("wgrad" + ("_s2" if six else ""))
                self.need(sW, self.lib.ksmi_up_wgrad_workspace(B, H, W, Cc))
                a_w = self._acc_param(wkey)
                self.bwd.add("ksmi_up_wgrad", lambda: (x.t.data_ptr(), gy.data_ptr(), self.scr(sW), self.m._g(wkey).data_ptr(), a_w, B, H, W, Cc),
                             {"kind": "up_gemm_wgrad", "bytes": B * H * W * Cc * 5 * es + 16 * Cc * Cc, "flops": 2 * B * H * W * Cc * 4 * Cc,
                              "tag": f"{wkey} K={Cc} N={4 * Cc} {H}x{W}", "side": True, "side_ix": six})
                self._mark(wkey)
            else:
                # weight gradient: G[tap d][k = n][col = c] -> grad[c*(4C) + n*4 + d]
                dw, ws = make_wgrad(s2, x.t, Cc, 0, Cc, self.m._g(wkey), 4, Cc * 4, 1, self._acc_param(wkey),
                                    B, 2 * H, 2 * W, H, W, 2, 2, 2, 0, self.dtype)
                self._wgrad(dw, ws, wkey)
            if not fused_bias:                                      # (no 3x3 consumer: separate pass over the gradient)
                npix = B * 4 * H * W
                rows = self._rows(npix)
                pb = torch.empty(rows * Cc, dtype=torch.float32, device=self.dev)
                self.bwd.add("ksmi_channel_sum", lambda: (gy.data_ptr(), pb.data_ptr(), rows, npix, Cc, self.dt))
                self._rowsum_at_end(bkey, pb, rows, 1, 0, Cc, Cc)
        self.bwd_builders.append((self.fwd.cur_lane, build_bwd))
        return y

    # ---------------------------------------------------------------- conv_block_nested  (snunet.py:11-29)
    def _block(self, name, branch, sources, out, first=False, pool=None):
        """pool: name of the max-pooled copy of the block output (encoder blocks, snunet.py:121-130).  With the fused BatchNorm glue
        (csrc/bnfused.hip) the pooled tensor comes out of the launch that writes the block output; returns (out, pooled) then."""
        m, B, H, W, Cc = self.m, out.B, out.H, out.W, out.C
        npix = B * H * W
        dtype, dt, training = self.dtype, self.dt, self.training
        self._level(H)
        i_act = Act(f"{name}{branch}.i", B, H, W, Cc, dtype, self.dev)
        z_act = Act(f"{name}{branch}.z", B, H, W, Cc, dtype, self.dev)
        sv1, sv2 = _Saved(Cc, self.dev), _Saved(Cc, self.dev)
        self.keep += [i_act, z_act, sv1, sv2]
        P = lambda s: m._p(f"{name}.{s}").data_ptr()
        G = lambda s: m._g(f"{name}.{s}").data_ptr()
        Bf = lambda s: m._b(f"{name}.{s}").data_ptr()
        Npad = conv_npad(Cc)
        sS, sR = self._sname("stats"), self._sname("red")             # per-lane scratch (this block's lane, forward and backward)
        stats = (lambda: self.scr(sS)) if training else (lambda: None)

        # ---- conv1 ----------------------------------------------------------------------
        if first:
            # forward: direct fp32 conv on the raw NCHW image (exact fp32 operands even in bf16 mode: quantising
            # the input image to bf16 costs ~2 points of gradient cosine downstream).  For the weight gradient
            # the image is also laid out as im2col [B,H,W,Kpad] (k = c*9+t) so dW runs on the MFMA wgrad kernel.
            x_img = sources[0]
            chead, cin = x_img.shape[1], m.in_channels
            x_tail = self.xtail.data_ptr() if self.tail else None
            kc = 32 if dtype == torch.bfloat16 else 16
            Kpad = -(-(cin * 9) // kc) * kc
            rows1, cpad1, Ktot = self.lib.ksmi_conv_first_stats_rows(B, H, W), Cc, cin
            self.need(sS, rows1 * 2 * Cc * 4)
            # raw tiles (model.set_input_pipeline): clamp / NaN / Normalize happen in the image load of both kernels
            raw = m._raw_ptrs(self.dev)
            self.fwd.add("ksmi_conv_first_forward_raw", lambda: (x_img.data_ptr(), x_tail, chead, P("conv1.weight"), P("conv1.bias"),
                                                                 i_act.t.data_ptr(), stats(), B, cin, H, W, Cc, *raw, dt))
            if self.with_backward:
                # the im2col image of the raw tile for the first-layer weight gradient is laid out in the BACKWARD list, right in front
                # of its only reader (the input buffers of the plan stay untouched until the next batch is set): the 103 MB it writes
                # are still in the 256 MB memory-side cache when the weight gradient reads them, and the forward pass does not carry them
                col = torch.empty((B, H, W, Kpad), dtype=dtype, device=self.dev)
                self.keep.append(col)
                im2col_args = lambda: (x_img.data_ptr(), x_tail, chead, col.data_ptr(), B, cin, H, W, Kpad, *raw, dt)
                if not self.im2col_late:
                    self.fwd.add("ksmi_im2col3x3_raw", im2col_args)
                src1 = [SrcSpec(col, Kpad)]
        else:
            srcs = [SrcSpec(a.t, a.C) for a in sources]
            Ktot = sum(a.C for a in sources)
            d1, t1 = make_conv(srcs, [(i_act.t, Cc, 0, 0, Cc, 0)], i_act.t, m._p(f"{name}.conv1.bias"), None,
                               B, H, W, H, W, 3, 3, 1, 1, Cc, dtype)
            w1 = self._packed(f"{name}.conv1.weight", t1, 9, Cc, Cc, 9, Ktot * 9, 0, 1, 0)
            d1.wpk = w1.data_ptr()
            rows1, cpad1 = conv_stats_rows(d1, dtype), Npad
            if training:
                self.need(sS, rows1 * 2 * Npad * 4)
                self.patch(d1, "stats", sS)
            self._conv(self.fwd, d1)

        gcount = float(npix * self.bn_world)                         # pixels the statistics describe (SyncBN: of all ranks)

        def bn_fin(bn, sv, rows, cpad):
            nbt = m._c(f"{name}.{bn}.num_batches_tracked").data_ptr()
            if self.sync_bn:                                          # rows of all ranks add up element-wise; the finish sums the rows
                self.fwd.add_allreduce(lambda rows=rows, cpad=cpad: self._bufs[sS][:rows * 2 * cpad * 4].view(torch.float32))
            self.fwd.add("ksmi_bn_finalize", lambda: (stats(), rows, cpad, Cc, gcount, P(f"{bn}.weight"), P(f"{bn}.bias"),
                                                      Bf(f"{bn}.running_mean"), Bf(f"{bn}.running_var"), nbt,
                                                      BN_MOMENTUM, BN_EPS, 1 if training else 0,
                                                      sv.mean, sv.rstd, sv.scale, sv.shift))
        bn_fin("bn1", sv1, rows1, cpad1)

        # ---- conv2 (BN1-apply + ReLU fused into the operand load) ---------------------------
        src2 = [SrcSpec(i_act.t, Cc, scale=sv1.scale_t, shift=sv1.shift_t, relu=1)]
        d2, t2 = make_conv(src2, [(z_act.t, Cc, 0, 0, Cc, 0)], z_act.t, m._p(f"{name}.conv2.bias"), None,
                           B, H, W, H, W, 3, 3, 1, 1, Cc, dtype)
        w2 = self._packed(f"{name}.conv2.weight", t2, 9, Cc, Cc, 9, Cc * 9, 0, 1, 0)
        d2.wpk = w2.data_ptr()
        rows2 = conv_stats_rows(d2, dtype)
        if training:
            self.need(sS, rows2 * 2 * Npad * 4)
            self.patch(d2, "stats", sS)
        self._conv(self.fwd, d2)
        fused = training and self.bn_fused and bool(self.lib.ksmi_bn_fused_supported(Cc, Npad, dt))
        pooled = None
        if fused:
            # statistics finish + BN2-apply + residual + ReLU (+ the 2x2 max-pool of the encoder blocks) in ONE launch
            if pool is not None:
                pooled = Act(pool, B, H // 2, W // 2, Cc, dtype, self.dev)
            nbt2 = m._c(f"{name}.bn2.num_batches_tracked").data_ptr()
            pp = pooled.t.data_ptr() if pooled is not None else None
            self.fwd.add("ksmi_bn_fin_add_relu", lambda: (stats(), rows2, Npad, Cc, float(npix), P("bn2.weight"), P("bn2.bias"),
                                                          Bf("bn2.running_mean"), Bf("bn2.running_var"), nbt2, BN_MOMENTUM, BN_EPS,
                                                          sv2.mean, sv2.rstd, sv2.scale, sv2.shift, z_act.t.data_ptr(), i_act.t.data_ptr(),
                                                          out.t.data_ptr(), pp, B, H, W, dt),
                         {"kind": "bn_fin_add_relu", "bytes": npix * Cc * self._es() * (3.25 if pooled is not None else 3), "flops": 0})
        else:
            bn_fin("bn2", sv2, rows2, Npad)
            self.fwd.add("ksmi_bn_add_relu", lambda: (z_act.t.data_ptr(), i_act.t.data_ptr(), sv2.scale, sv2.shift,
                                                      out.t.data_ptr(), npix, Cc, dt))

        # ---- backward ----------------------------------------------------------------------------
        def build_bwd():
            self._level(H)
            # (the virtual-sum input gradient below is the last writer of d out: the other producers -- pool / Up input gradients, the
            # ECAM head -- belong to modules later in the forward order, i.e. earlier in this list)
            gated = self._emit_dgrad(out, gate=(out.t, z_act.t, sv2)) if os.environ.get("KSMI_NO_GATE") is None else self._emit_dgrad(out)
            gated = gated if isinstance(gated, tuple) else None
            rows = self._rows(npix)
            self.need(sR, rows * 2 * Cc * 4)
            sums1 = torch.zeros((2, Cc), dtype=torch.float32, device=self.dev)
            sums2 = torch.zeros((2, Cc), dtype=torch.float32, device=self.dev)
            dz = torch.empty_like(z_act.t)     # grad wrt conv2 output
            r = torch.empty_like(i_act.t)      # relu-masked dgrad of conv2, then di (grad wrt conv1 output)
            self.keep += [sums1, sums2, dz, r]
            gout = out.grad().data_ptr()
            s1p, s2p = sums1.data_ptr(), sums2.data_ptr()
            a_bn2 = self._acc_param(f"{name}.bn2")
            es = self._es()
            if gated is not None:
                # d out arrives gated (x (out > 0)) with the BatchNorm2-backward sums in the statistics rows of its producer
                gst, grows, gpad = gated
                if fused and self.lib.ksmi_bn_fused_supported(Cc, gpad, dt):
                    self.bwd.add("ksmi_bn_bwd_fin_apply_gated", lambda: (gst.data_ptr(), grows, gpad, s2p, G("bn2.weight"), G("bn2.bias"), a_bn2,
                                                                         gout, z_act.t.data_ptr(), sv2.mean, sv2.rstd, P("bn2.weight"),
                                                                         dz.data_ptr(), float(npix), npix, Cc, dt),
                                 {"kind": "bn_bwd_fin_apply_gated", "bytes": npix * Cc * es * 3, "flops": 0})
                    self._mark(f"{name}.bn2.weight", f"{name}.bn2.bias")
                else:
                    self.bwd.add("ksmi_reduce_rows", lambda: (gst.data_ptr(), grows, 2, gpad, Cc, s2p, G("bn2.weight"), G("bn2.bias"), a_bn2))
                    self._mark(f"{name}.bn2.weight", f"{name}.bn2.bias")
                    if self.sync_bn:          # (the parameter gradients above stay LOCAL sums: the gradient all-reduce adds them; d x needs the global ones)
                        self.bwd.add_allreduce(lambda: sums2)
                    self.bwd.add("ksmi_bn_bwd_apply_gated", lambda: (gout, z_act.t.data_ptr(), sv2.mean, sv2.rstd, P("bn2.weight"), s2p,
                                                                     dz.data_ptr(), gcount, npix, Cc, dt))
            else:
                self.bwd.add("ksmi_bnrelu_bwd_reduce", lambda: (gout, out.t.data_ptr(), z_act.t.data_ptr(), sv2.mean, sv2.rstd,
                                                                self.scr(sR), rows, npix, Cc, dt))
                if fused:
                    self.bwd.add("ksmi_bnrelu_bwd_fin_apply", lambda: (self.scr(sR), rows, Cc, s2p, G("bn2.weight"), G("bn2.bias"), a_bn2,
                                                                       gout, out.t.data_ptr(), z_act.t.data_ptr(), sv2.mean, sv2.rstd,
                                                                       P("bn2.weight"), dz.data_ptr(), float(npix), npix, Cc, dt),
                                 {"kind": "bnrelu_bwd_fin_apply", "bytes": npix * Cc * es * 5, "flops": 0})
                    self._mark(f"{name}.bn2.weight", f"{name}.bn2.bias")
                else:
                    self.bwd.add("ksmi_reduce_rows", lambda: (self.scr(sR), rows, 2, Cc, Cc, s2p, G("bn2.weight"), G("bn2.bias"), a_bn2))
                    self._mark(f"{name}.bn2.weight", f"{name}.bn2.bias")
                    if self.sync_bn:
                        self.bwd.add_allreduce(lambda: sums2)
                    self.bwd.add("ksmi_bnrelu_bwd_apply", lambda: (gout, out.t.data_ptr(), z_act.t.data_ptr(), sv2.mean, sv2.rstd,
                                                                   P("bn2.weight"), s2p, dz.data_ptr(), gcount, npix, Cc, dt))
            # conv2.bias feeds a train-mode BatchNorm: its gradient sum(dz) is analytically 0 (the reference holds
            # ~1e-6 of rounding noise there); write exact zeros instead of two reduction launches.
            if training:
                self._rowsum_at_end(f"{name}.conv2.bias", None, 0, 1, 0, Cc, Cc)
            else:                                                   # eval-mode BN: d bias = sum(dz)
                pz = torch.empty(rows * Cc, dtype=torch.float32, device=self.dev)
                self.bwd.add("ksmi_channel_sum", lambda: (dz.data_ptr(), pz.data_ptr(), rows, npix, Cc, dt))
                self._rowsum_at_end(f"{name}.conv2.bias", pz, rows, 1, 0, Cc, Cc)
            # dgrad of conv2 with fused ReLU mask + BN1-backward statistics in the epilogue
            dg2, tg2 = make_conv([SrcSpec(dz, Cc)], [(r, Cc, 0, 0, Cc, 0)], dz, None, None, B, H, W, H, W, 3, 3, 1, 1, Cc, dtype,
                                 mask=(i_act.t, sv1.t[0], sv1.t[1], sv1.t[2], sv1.t[3]))
            wg2 = self._packed(f"{name}.conv2.weight", tg2, 9, Cc, Cc, Cc * 9, 9, 0, 1, 1)
            dg2.wpk = wg2.data_ptr()
            rows_g = conv_stats_rows(dg2, dtype)
            self.need(sS, rows_g * 2 * Npad * 4)
            self.patch(dg2, "stats", sS)
            self._conv(self.bwd, dg2, "dgrad")
            a_bn1 = self._acc_param(f"{name}.bn1")
            if not fused:
                self.bwd.add("ksmi_reduce_rows", lambda: (self.scr(sS), rows_g, 2, Npad, Cc, s1p, G("bn1.weight"), G("bn1.bias"), a_bn1))
                self._mark(f"{name}.bn1.weight", f"{name}.bn1.bias")
                if self.sync_bn:
                    self.bwd.add_allreduce(lambda: sums1)
            # weight gradient of conv2: X = relu(bn1(i)) recomputed on load, dY = dz
            dw2, ws2 = make_wgrad(src2, dz, Cc, 0, Cc, m._g(f"{name}.conv2.weight"), 9, Cc * 9, 1,
                                  self._acc_param(f"{name}.conv2.weight"), B, H, W, H, W, 3, 3, 1, 1, dtype)
            self._wgrad(dw2, ws2, f"{name}.conv2.weight")
            # di = g + BN1 backward (over r, in place); conv1 bias gradient
            pb1 = torch.empty(rows * Cc, dtype=torch.float32, device=self.dev)      # per-block partial sums of di (conv1 bias gradient)
            if fused:
                # the BN1-backward sums are finished from the statistics rows of conv2's input gradient inside the apply pass.  (The
                # weight gradient of conv2 above runs on the side stream and does not touch `stats`; nothing else of this lane writes
                # the rows between the two launches.)
                rows_b = min(rows, self.lib.ksmi_bn_fused_max_rows())
                self.bwd.add("ksmi_bn_bwd_fin_apply_add", lambda: (self.scr(sS), rows_g, Npad, s1p, G("bn1.weight"), G("bn1.bias"), a_bn1,
                                                                   r.data_ptr(), gout, i_act.t.data_ptr(), sv1.mean, sv1.rstd, P("bn1.weight"),
                                                                   pb1.data_ptr(), rows_b, float(npix), npix, Cc, dt),
                             {"kind": "bn_bwd_fin_apply_add", "bytes": npix * Cc * self._es() * 4, "flops": 0})
                self._mark(f"{name}.bn1.weight", f"{name}.bn1.bias")
                self._rowsum_at_end(f"{name}.conv1.bias", pb1, rows_b, 1, 0, Cc, Cc)
            else:
                self.bwd.add("ksmi_bn_bwd_apply_add", lambda: (r.data_ptr(), gout, i_act.t.data_ptr(), sv1.mean, sv1.rstd,
                                                               P("bn1.weight"), s1p, pb1.data_ptr(), rows, gcount, npix, Cc, dt))
                self._rowsum_at_end(f"{name}.conv1.bias", pb1, rows, 1, 0, Cc, Cc)
            a_w1 = self._acc_param(f"{name}.conv1.weight")
            if first:
                # dW[n][c*9+t] = sum_px im2col[px][c*9+t] * di[px][n]  (1x1 weight-gradient GEMM over the saved im2col)
                if self.im2col_late:
                    self.bwd.add("ksmi_im2col3x3_raw", im2col_args, {"kind": "im2col3x3_raw", "bytes": B * H * W * (cin * 4 + Kpad * self._es()), "flops": 0})
                dw1, ws1 = make_wgrad(src1, r, Cc, 0, Cc, m._g(f"{name}.conv1.weight"), 1, cin * 9, 0, a_w1,
                                      B, H, W, H, W, 1, 1, 1, 0, dtype)
                for ci in range(dw1.nchunks):
                    dw1.k_len[ci] = max(0, min(dw1.k_len[ci], cin * 9 - dw1.k_off[ci]))
                self._wgrad(dw1, ws1, f"{name}.conv1.weight")
            else:
                srcs = [SrcSpec(a.t, a.C) for a in sources]
                # input gradients are NOT launched here: every source registers this block's `di` as one of
                # its consumers and its producer gathers all of them in ONE "virtual sum" dgrad (_emit_dgrad)
                nb = 0
                for a in sources:
                    a.consumers.append((r, Cc, f"{name}.conv1.weight", nb, Ktot))
                    nb += a.C
                dw1, ws1 = make_wgrad(srcs, r, Cc, 0, Cc, m._g(f"{name}.conv1.weight"), 9, Ktot * 9, 1, a_w1,
                                      B, H, W, H, W, 3, 3, 1, 1, dtype)
                self._wgrad(dw1, ws1, f"{name}.conv1.weight")
        self.bwd_builders.append((self.fwd.cur_lane, build_bwd))
        if pool is not None:
            return out, pooled           # pooled = None: the caller's _pool_at() launches the stand-alone max-pool
        return out

    # ---------------------------------------------------------------- ECAM head  (snunet.py:49-62,146-151)
    def _head(self, xs):
        m, B, n = self.m, self.B, self.n
        HW = self.H * self.W
        dev, dt = self.dev, self.dt
        self._stage("head")
        f32 = dict(dtype=torch.float32, device=dev)
        avg, mx = torch.zeros((B, 5 * n), **f32), torch.zeros((B, 5 * n), **f32)
        argmax = torch.zeros((B, 5 * n), dtype=torch.int32, device=dev)
        ca, ca1 = torch.zeros((B, 4 * n), **f32), torch.zeros((B, n), **f32)
        hidden = torch.zeros((B, 2, 4 * n // 16 + n // 4), **f32)
        xarr = (C.c_void_p * 4)(*[a.t.data_ptr() for a in xs])
        ws_pool = torch.empty(self.lib.ksmi_ecam_pool_workspace(B, HW, n), dtype=torch.uint8, device=dev)
        self.keep += [avg, mx, argmax, ca, ca1, hidden, xarr, ws_pool]
        self.head = dict(avg=avg, mx=mx, argmax=argmax, ca=ca, ca1=ca1)
        P = lambda key: m._p(key).data_ptr()
        G = lambda key: m._g(key).data_ptr()
        T0 = B * HW * n * self._es()             # one [B,H,W,n] map
        self.fwd.add("ksmi_ecam_pool", lambda: (xarr, avg.data_ptr(), mx.data_ptr(), argmax.data_ptr(), ws_pool.data_ptr(), B, HW, n, dt),
                     {"kind": "ecam_pool", "bytes": 4 * T0, "flops": 0})
        self.fwd.add("ksmi_ecam_mlp", lambda: (avg.data_ptr(), mx.data_ptr(), P("ca.fc1.weight"), P("ca.fc2.weight"),
                                               P("ca1.fc1.weight"), P("ca1.fc2.weight"), ca.data_ptr(), ca1.data_ptr(),
                                               hidden.data_ptr(), B, n))
        self.fwd.add("ksmi_ecam_final_forward", lambda: (xarr, ca.data_ptr(), ca1.data_ptr(), P("conv_final.weight"),
                                                         P("conv_final.bias"), self.logits.data_ptr(), B, HW, n, 3, dt),
                     {"kind": "ecam_final_forward", "bytes": 4 * T0 + B * HW * 3 * 4, "flops": 2 * B * HW * 4 * n * 3})

        def build_bwd():
            self._stage("head")
            dca, dca1 = torch.zeros((B, 4 * n), **f32), torch.zeros((B, n), **f32)
            davg, dmax = torch.zeros((B, 5 * n), **f32), torch.zeros((B, 5 * n), **f32)
            ws_b = torch.empty(self.lib.ksmi_ecam_bwd_workspace(B, HW, n, 3), dtype=torch.uint8, device=dev)
            ws_m = torch.empty(self.lib.ksmi_ecam_mlp_bwd_workspace(B, n), dtype=torch.uint8, device=dev)
            garr = (C.c_void_p * 4)(*[a.grad().data_ptr() for a in xs])
            for a in xs:
                a.take_acc_flag()
            for key in ("conv_final.weight", "conv_final.bias", "ca.fc1.weight", "ca.fc2.weight", "ca1.fc1.weight", "ca1.fc2.weight"):
                self._acc_param(key)
            self.keep += [dca, dca1, davg, dmax, ws_b, ws_m, garr]
            dl = self.dlogits.data_ptr()
            self.bwd.add("ksmi_ecam_final_backward_reduce", lambda: (
                xarr, dl, ca.data_ptr(), ca1.data_ptr(), P("conv_final.weight"), dca.data_ptr(), dca1.data_ptr(),
                G("conv_final.weight"), G("conv_final.bias"), ws_b.data_ptr(), B, HW, n, 3, dt),
                {"kind": "ecam_final_backward_reduce", "bytes": 4 * T0 + B * HW * 3 * 4, "flops": 2 * B * HW * 4 * n * 3})
            self._mark("conv_final.weight", "conv_final.bias")
            self.bwd.add("ksmi_ecam_mlp_backward", lambda: (
                avg.data_ptr(), mx.data_ptr(), hidden.data_ptr(), ca.data_ptr(), ca1.data_ptr(), dca.data_ptr(), dca1.data_ptr(),
                P("ca.fc1.weight"), P("ca.fc2.weight"), P("ca1.fc1.weight"), P("ca1.fc2.weight"), davg.data_ptr(), dmax.data_ptr(),
                G("ca.fc1.weight"), G("ca.fc2.weight"), G("ca1.fc1.weight"), G("ca1.fc2.weight"), ws_m.data_ptr(), B, n))
            self._mark("ca.fc1.weight", "ca.fc2.weight", "ca1.fc1.weight", "ca1.fc2.weight")
            self.bwd.add("ksmi_ecam_final_backward_dx", lambda: (
                garr, dl, ca.data_ptr(), P("conv_final.weight"), davg.data_ptr(), dmax.data_ptr(), argmax.data_ptr(), B, HW, n, 3, dt),
                {"kind": "ecam_final_backward_dx", "bytes": 4 * T0 + B * HW * 3 * 4, "flops": 2 * B * HW * 4 * n * 3})
        self.bwd_builders.append((self.fwd.cur_lane, build_bwd))

    # ---------------------------------------------------------------- execution
    def run_forward(self, xA, xB, tail=None):
        if (tail is None) != (self.xtail is None):
            raise _lib.KsmiError("plan and call disagree about the shared tail channels (DEM)")
        return self._run_forward(self.logits, (xA, self.xA), (xB, self.xB), *([] if tail is None else [(tail, self.xtail)]))
