"""The launch-list executor shared by every model plan and train step: LaunchList = the prepared C-ABI calls of a plan, walked either
in Python or as a compiled `ksmi_op` array by ONE ksmi_run_list call per segment (csrc/runlist.hip); StepStreams = the HIP streams of
one train step (main / second compute lane / side streams) and the ordering state between them."""
import ctypes as C
import os

import torch

from . import _lib
from .runtime import stream_ptr


_TAG_IDS = {}


def _tag_id(tag):
    """side-stream tags of the plans (arbitrary hashables) as the small integers ksmi_op carries"""
    return _TAG_IDS.setdefault(tag, len(_TAG_IDS))


def _slot(code, v, struct):
    """one prepared argument as the 64-bit slot the call thunks read (include/ksmi.h ksmi_op)"""
    if hasattr(v, "value") and not hasattr(v, "_obj"):        # a ctypes scalar (c_void_p, c_int, ...)
        v = v.value
    if code == "p":
        if v is None:
            return 0
        if isinstance(v, int):
            return v
        if hasattr(v, "_obj"):                                # ctypes.byref(x)
            return C.addressof(v._obj)
        if isinstance(v, (C.Array, C.Structure)):
            return C.addressof(v)
        if isinstance(v, C._Pointer):
            return C.cast(v, C.c_void_p).value or 0
        raise _lib.KsmiError(f"launch list: cannot take the address of a {type(v).__name__} argument")
    if code == "f":
        return struct.unpack("<I", struct.pack("<f", float(v)))[0]
    if code == "d":
        return struct.unpack("<Q", struct.pack("<d", float(v)))[0]
    return int(v) & 0xFFFFFFFFFFFFFFFF


_PLAIN_RUNNERS = {}


def _plain_runner(st):
    """the executor state of single-stream runs (model(x) outside a train step): everything on the caller's current stream"""
    dev = torch.cuda.current_device() if torch.cuda.is_available() else -1
    lib = _lib.load()
    r = _PLAIN_RUNNERS.get(dev)
    if r is None:
        r = _PLAIN_RUNNERS[dev] = C.c_void_p(lib.ksmi_runner_create())
    lib.ksmi_runner_set_streams(r, st, None, None, None)
    return r


class LaunchList:
    """(name, argfn, meta) triples; argfn() is evaluated once, after all scratch buffers exist.
    meta = {"kind": kernel class, "bytes": algorithmic HBM bytes, "flops": 2*MAC} for the roofline, plus the scheduling tags
    "lane" (compute lane the launch belongs to: 0 = the caller's stream, 1 = the second lane) and "side" (weight gradient: may
    run on the side stream).  ("@wait", (a, b)) entries order lane b behind everything lane a was handed so far."""

    def __init__(self):
        self.pending, self.calls = [], []
        self.cur_lane = 0
        self.cur_stage = None      # measurement tag of the launches appended from here on (bench.py roofline.stages)

    def add(self, name, argfn, meta=None):
        meta = dict(meta) if meta else {"kind": name[5:], "bytes": 0, "flops": 0}
        meta["lane"] = self.cur_lane
        meta.setdefault("stage", self.cur_stage)
        self.pending.append((name, argfn, meta))

    def add_wait(self, src, dst):
        self.pending.append(("@wait", lambda: (src, dst), {"kind": "wait", "bytes": 0, "flops": 0, "lane": dst}))

    def add_allreduce(self, tensor_fn, meta=None):
        """SyncBN (optional): SUM `tensor_fn()` (a small fp32 statistics tensor) over the ranks, in place, on the stream of
        the issuing lane, between the launch that wrote it and the launch that reads it"""
        m = {"kind": "syncbn_allreduce", "bytes": 0, "flops": 0, "lane": self.cur_lane}
        m.setdefault("stage", self.cur_stage)
        self.pending.append(("@allreduce", lambda: (tensor_fn(),), m | (meta or {})))

    def add_wait_side(self, tag=None):
        """the issuing lane waits for the side-stream launch that carries meta["side_tag"] == tag (None: for everything handed to the
        side stream so far): placed before a launch that overwrites an operand of that weight gradient (plans that recycle buffers)"""
        self.pending.append(("@wait_side", lambda: (tag,), {"kind": "wait", "bytes": 0, "flops": 0, "lane": self.cur_lane}))

    def resolve(self, lib):
        self.calls = [(None if name.startswith("@") else getattr(lib, name), tuple(argfn()), name, meta) for name, argfn, meta in self.pending]
        self._compiled = None          # (the compiled form holds the argument values of the previous resolution)

    # ---- compiled form (round 6): the list as an array of ksmi_op walked by ONE C-ABI call per segment (csrc/runlist.hip) instead of one
    # ctypes call + stream switch + up to three torch event calls per launch in Python (host_issue_ms_per_step: 9 ms of a 14 ms SNUNet
    # step, 29 of 34 ms for ChangeFormer).  The Python walk below stays for timed runs (a kernel timer brackets single launches), for hooks
    # without an index list, for SyncBN's collectives, and as the cross-check (KSMI_RUN_LIST=0; tests/test_gpu_graph.py).  Both walks take
    # every cross-stream edge from the step's one runner (StepStreams.runner), so the lists of one step may mix them.
    fast = os.environ.get("KSMI_RUN_LIST", "1") != "0"
    _compiled = None

    def _compile(self):
        import struct
        lib = _lib.load()
        n = len(self.calls)
        ops = (_lib.Op * max(n, 1))()
        slots, where, skips, names, ok = [], [], [], [], True
        for i, (fn, args, name, meta) in enumerate(self.calls):
            op = ops[i]
            op.tag, op.sig = -1, -1
            op.lane = int(meta.get("lane", 0))
            names.append(name)
            if fn is None:
                if name == "@wait":
                    op.kind, op.a, op.b = _lib.OP_ORDER, int(args[0]), int(args[1])
                elif name == "@wait_side":
                    op.kind, op.tag = _lib.OP_WAIT_SIDE, (-1 if args[0] is None else _tag_id(args[0]))
                else:
                    ok = False                   # ("@allreduce": SyncBN's collectives are issued by torch.distributed)
                continue
            if name not in _lib.SIGNATURES:       # (a stubbed library in the host-only tests: the Python walk)
                ok = False
                continue
            restype, argtypes = _lib.SIGNATURES[name]
            codes = _lib.sig_codes(argtypes[:-1])
            sig = lib.ksmi_thunk_id(codes.encode())
            if sig < 0 or len(codes) != len(args):
                raise _lib.KsmiError(f"launch list: no call thunk for {name} ({codes!r}, {len(args)} arguments): re-run tools/gen_thunks.py")
            op.kind, op.sig, op.nargs = _lib.OP_CALL, sig, len(args)
            op.fn = C.cast(fn, C.c_void_p).value
            op.side = (2 if meta.get("side_ix", 0) else 1) if meta.get("side") else 0
            if op.side and meta.get("side_tag") is not None:
                op.tag = _tag_id(meta["side_tag"])
            where.append((i, len(slots)))
            slots += [_slot(c, v, struct) for c, v in zip(codes, args)]
            if meta.get("skip_if") is not None:
                skips.append((i, meta["skip_if"]))
        arr = (C.c_uint64 * max(len(slots), 1))(*slots)
        base = C.addressof(arr)
        for i, off in where:
            ops[i].args = base + 8 * off
        self._compiled = {"ops": ops, "slots": arr, "n": n, "skips": skips, "names": names, "ok": ok, "failed": C.c_int32(-1),
                          "skipbuf": (C.c_uint8 * max(n, 1))() if skips else None}
        return self._compiled

    def _run_fast(self, hook, hook_at, streams):
        cp = self._compiled
        lib = _lib.load()
        if streams is not None:
            streams.begin()
            runner = streams.runner()
        else:
            runner = _plain_runner(stream_ptr())
        skip = None
        if cp["skips"]:
            skip = cp["skipbuf"]
            for i, fn in cp["skips"]:
                skip[i] = 1 if fn() else 0
        n = cp["n"]
        cuts = sorted({i + 1 for i in hook_at if 0 <= i < n} | {n}) if hook is not None else [n]
        a = 0
        for b in cuts:
            rc = lib.ksmi_run_list(runner, cp["ops"], a, b, skip, C.byref(cp["failed"]))
            if rc != 0:
                at = cp["failed"].value
                _lib.check(rc, cp["names"][at] if 0 <= at < n else "ksmi_run_list")
            if hook is not None and (b - 1) in hook_at:
                hook(b - 1)
            a = b

    def run(self, timer=None, hook=None, streams=None, hook_at=None):
        """hook_at: the list indices at which `hook` has work to do (dp.BucketedAllReduce.hook_indices); with it (or without a hook) and
        without a timer the compiled list runs (see above).
        streams = StepStreams or None.  None: every launch on the current stream, in list order (always a valid order; the
        "@wait" entries are no-ops).  With streams: launches of lane 1 go to the second compute stream, launches tagged "side" (the
        weight gradients: nothing on the critical path of the backward pass reads them) to the side stream behind an event recorded
        on the issuing lane's stream at that point of the list, so that independent work fills the machine next to the
        bandwidth-bound BatchNorm / elementwise launches of the critical path; the caller joins (StepStreams.join / end) before
        anything outside the lists reads the results.  The walk below makes the launches and the stream switches; the forks, tagged
        events and waits are the runner's (StepStreams.order / fork_side / mark_side / wait_side), as in the compiled walk."""
        if (timer is None or not getattr(timer, "active", True)) and self.fast and self.calls and (hook is None or hook_at is not None):
            cp = self._compiled or self._compile()
            if cp["ok"]:
                return self._run_fast(hook, hook_at or (), streams)
        if streams is not None:
            streams.begin()
        st, cur = stream_ptr(), 0
        try:
            for idx, (fn, args, name, meta) in enumerate(self.calls):
                if fn is None and name == "@allreduce":
                    lane = meta["lane"] if streams is not None and streams.lanes else 0
                    if lane != cur:
                        torch.cuda.set_stream(streams.stream(lane))
                        st, cur = stream_ptr(), lane
                    from . import distributed as D
                    D.all_reduce_sum_(args[0])                       # (stream-ordered on RCCL; gloo stages through the host)
                    if hook is not None:
                        hook(idx)
                    continue
                if fn is None:
                    if name == "@wait_side":
                        if streams is not None and streams.use_side:
                            streams.wait_side(args[0], meta["lane"] if streams.lanes else 0, cur)
                    elif streams is not None and streams.lanes:
                        streams.order(*args)
                    if hook is not None:
                        hook(idx)
                    continue
                if meta.get("skip_if") is not None and meta["skip_if"]():      # (plan_base: the bf16 mirror the optimiser just wrote)
                    continue
                lane = meta["lane"] if streams is not None and streams.lanes else 0
                if lane != cur:
                    torch.cuda.set_stream(streams.stream(lane))
                    st, cur = stream_ptr(), lane
                timed = timer is not None and timer.wants(meta["kind"])
                if timed:
                    timer.begin(meta["kind"], meta)
                if streams is not None and streams.use_side and not timed and meta.get("side"):     # (a timed launch is bracketed by events on its lane's stream)
                    six = 1 if meta.get("side_ix", 0) else 0
                    rc = fn(*args, streams.fork_side(lane, six))
                    if rc == 0 and meta.get("side_tag") is not None:
                        streams.mark_side(meta["side_tag"], six)
                else:
                    rc = fn(*args, st)
                if timed:
                    timer.end()
                if rc != 0:
                    _lib.check(rc, name)
                if hook is not None:
                    hook(idx)
        finally:
            if cur != 0:
                torch.cuda.set_stream(streams.main)


class StepStreams:
    """The HIP streams of one train step: main = the caller's current stream (lane 0), lane1 = a second compute lane for the
    deeper decoder blocks (SNUNetPlan: they depend on the level-0 blocks only through the Up1_j edges), side = the weight gradients.
    Cross-stream ordering is plain event record / wait pairs, so a step that uses them still captures into one HIP graph.  The
    ordering state (fork events, tagged events, busy / dirty flags) lives in ONE place, the runner of csrc/runlist.hip: the compiled
    walk drives it from C, the Python walk through order / fork_side / mark_side / wait_side below."""

    def __init__(self, device, lanes=True, side=True):
        self.side = torch.cuda.Stream(device=device)       # (stream priorities measured no better)
        # KSMI_SIDE2=1 (experiment): a second side stream; the SNUNet plan alternates its weight gradients between the two by parameter
        # (meta["side_ix"]: launches that accumulate into one gradient stay on one stream), so the slab reducer of one weight gradient
        # runs beside the main kernel of the next
        self.side2 = torch.cuda.Stream(device=device) if (side and os.environ.get("KSMI_SIDE2", "0") == "1") else None
        self.side2_ptr = C.c_void_p(self.side2.cuda_stream) if self.side2 is not None else None
        self.lane1 = torch.cuda.Stream(device=device) if lanes else None
        self.lanes, self.use_side = bool(lanes), bool(side)
        self.side_ptr = C.c_void_p(self.side.cuda_stream)
        self.main = None

    # (class attributes: an object that never asked for a runner carries neither, and __del__ may run on one that __init__ never finished)
    _runner = None
    _runner_pid = None      # the process that created the runner: only that one destroys it (see __del__)

    def begin(self):
        if self.main is None:
            self.main = torch.cuda.current_stream()
            if self._runner is not None:
                self._bind_runner()

    def _bind_runner(self):
        _lib.load().ksmi_runner_set_streams(self._runner, C.c_void_p(self.main.cuda_stream),
                                            C.c_void_p(self.lane1.cuda_stream) if self.lanes else None,
                                            self.side_ptr if self.use_side else None, self.side2_ptr if self.use_side else None)

    def runner(self):
        """executor state (csrc/runlist.hip) bound to this step's streams, created at its first use; call after begin()"""
        if self._runner is None:
            self._runner = C.c_void_p(_lib.load().ksmi_runner_create())
            self._runner_pid = os.getpid()
            self._bind_runner()
        return self._runner

    def __del__(self):
        # only in the process that created the runner: a forked DataLoader worker that collects an inherited copy of this object
        # must not call hipEventDestroy (the HIP runtime does not survive a fork: the worker dies with a segmentation fault)
        try:
            if self._runner is not None and self._runner_pid == os.getpid():
                _lib.load().ksmi_runner_destroy(self._runner)
        except Exception:
            pass

    def stream(self, lane):
        return self.main if lane == 0 else self.lane1

    def order(self, src, dst):
        _lib.check(_lib.load().ksmi_runner_order(self.runner(), src, dst), "ksmi_runner_order")

    def fork_side(self, lane, ix=0):
        """side stream `ix` waits for what `lane` was handed so far; returns the stream the weight gradient goes to"""
        out = C.c_void_p()
        _lib.check(_lib.load().ksmi_runner_fork_side(self.runner(), lane, ix, C.byref(out)), "ksmi_runner_fork_side")
        return out

    def mark_side(self, tag, ix=0):
        _lib.check(_lib.load().ksmi_runner_mark_side(self.runner(), _tag_id(tag), ix), "ksmi_runner_mark_side")

    def wait_side(self, tag, lane, cur):
        """the entry's lane and the lane of the last launch wait for the side launch tagged `tag` (None: for the side streams, if busy)"""
        _lib.check(_lib.load().ksmi_runner_wait_side(self.runner(), lane, cur, -1 if tag is None else _tag_id(tag)), "ksmi_runner_wait_side")

    def all_streams(self):
        """every stream a launch of the step may have run on"""
        return [s for s in (self.main, self.lane1 if self.lanes else None, self.side if self.use_side else None,
                            self.side2 if self.use_side else None) if s is not None]

    def join(self):
        """main waits for every other stream of the step that was handed work (by either walk), and the caller's current stream, if it
        is another one, for main"""
        if self._runner is not None:
            _lib.check(_lib.load().ksmi_runner_join(self._runner), "ksmi_runner_join")
        if self.main is not None:
            cur = torch.cuda.current_stream()
            if cur.cuda_stream != self.main.cuda_stream:
                cur.wait_stream(self.main)

    def end(self):
        self.join()
        self.main = None
