"""CPU: host-side mirror of the reference's operator surface (config derivation table of
SURVEY.md §8(c), JSON5 loader, synthetic batch contract, checkpoint directory naming, metrics
oracle hand cases)."""
import os

import numpy as np
import pytest
import torch

from kurosiwo_amd.config import create_checkpoint_directory, load_json5, update_config
from kurosiwo_amd.synthetic import cd_inputs, make_batch
from oracle import metrics_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Args:
    def __init__(self, inputs=None, dem=False, slope=False):
        self.inputs, self.dem, self.slope = inputs, dem, slope


def _cfg(task, **kw):
    c = load_json5(os.path.join(ROOT, "configs/config.json"))
    c.update(load_json5(os.path.join(ROOT, "configs/method/snunet/snunet.json")))
    c["task"] = task
    c = update_config(c, Args(**kw), root=ROOT)
    return c


def test_num_channels_table():
    # cd/GRD 2, cd/GRD+dem 3, seg 3-date GRD 6, seg 3-date+dem 7 (utilities.py:377-390)
    assert _cfg("cd", inputs=["pre_event_1", "post_event"])["num_channels"] == 2
    assert _cfg("cd", inputs=["pre_event_1", "post_event"], dem=True)["num_channels"] == 3
    assert _cfg("segmentation")["num_channels"] == 6
    assert _cfg("segmentation", inputs=["pre_event_1", "pre_event_2", "post_event"], dem=True)["num_channels"] == 7
    c = _cfg("cd", inputs=["pre_event_1", "post_event"])
    assert c["class_weights"] == [1.0, 1.0, 1.0] and c["device"] == "cuda:0" and c["inputs"] == ["pre_event_1", "post_event"]


def test_json5_loader_handles_comments_and_trailing_commas(tmp_path):
    p = tmp_path / "c.json"
    p.write_text('{\n "a": 1, // comment with "quotes"\n "url": "http://x//y", // keep\n "l": [1,2,],\n}\n')
    assert load_json5(p) == {"a": 1, "url": "http://x//y", "l": [1, 2]}


def test_json5_loader_reads_reference_config_files(golden_dir):
    ref = os.path.join(golden_dir, "reference_configs")         # the reference's own config files, stored verbatim
    c = load_json5(os.path.join(ref, "config.json"))
    assert c["num_classes"] == 3 and c["task"] == "segmentation"
    d = load_json5(os.path.join(ref, "train/data_config.json"))
    mine = load_json5(os.path.join(ROOT, "configs/train/data_config.json"))
    for k in ("data_mean", "data_std", "dem_mean", "dem_std", "clamp_input", "inputs", "channels", "train_acts", "val_acts", "test_acts"):
        assert d[k] == mine[k], k
    s = load_json5(os.path.join(ref, "method/snunet/snunet.json"))
    m = load_json5(os.path.join(ROOT, "configs/method/snunet/snunet.json"))
    assert s == {k: m[k] for k in s}


def test_synthetic_batch_contract():
    b = make_batch(3, 32, 32, seed=5)
    assert len(b) == 12
    assert b[2].shape == (3, 2, 32, 32) and b[3].shape == (3, 32, 32) and b[3].dtype == torch.int64
    assert isinstance(b[0], list) and b[0][0].dtype == torch.float64 and b[0][0].shape == (3,)
    assert set(b[3].unique().tolist()) <= {0, 1, 2, 3}
    vv = b[2][:, 0]
    assert float(vv.min()) >= -2.24 and float(vv.max()) <= 1.29          # SURVEY.md §8(d) value range
    bd = make_batch(2, 32, 32, seed=5, dem=True)
    assert len(bd) == 13 and bd[10].shape == (2, 1, 32, 32)
    (xA, xB), mask = cd_inputs(bd, ("pre_event_1", "post_event"), dem=True)
    assert xA.shape == (2, 3, 32, 32) and torch.equal(xB[:, :2], bd[2])
    b2 = make_batch(3, 32, 32, seed=5)
    assert torch.equal(b[2], b2[2]) and torch.equal(b[3], b2[3])


def test_checkpoint_directory_naming(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    p = create_checkpoint_directory({"task": "cd", "method": "SNUNet", "track": "RandomEvents"}, {})
    assert p.startswith("checkpoints/snunet/RandomEvents_") and os.path.isdir(p)


def test_metrics_oracle_hand_cases():
    # hand-computed confusion-matrix cases (torchmetrics semantics; parity unpinned by import)
    pred = np.array([0, 1, 2, 2, 1, 0, 0, 3])
    tgt = np.array([0, 1, 2, 1, 3, 2, 0, 0])
    cm = metrics_ref.confusion_matrix(pred, tgt)
    assert cm.sum() == 7 and cm[3].sum() == 0          # target==3 dropped
    assert cm[0, 0] == 2 and cm[0, 3] == 1 and cm[1, 1] == 1 and cm[1, 2] == 1 and cm[2, 2] == 1 and cm[2, 0] == 1
    m = metrics_ref.metrics_from_cm(cm)
    assert np.allclose(m["recall"], [2 / 3, 1 / 2, 1 / 2, 0.0])
    assert np.allclose(m["precision"], [2 / 3, 1.0, 1 / 2, 0.0])
    assert np.allclose(m["iou"], [2 / 4, 1 / 2, 1 / 3, 0.0])
    assert abs(m["miou"] - (0.5 + 0.5 + 1 / 3) / 3) < 1e-12
    from kurosiwo_amd.metrics import metrics_from_cm
    mm = metrics_from_cm(torch.tensor(cm))
    for k in ("accuracy", "precision", "recall", "f1", "iou"):
        assert np.allclose(mm[k].numpy(), m[k])


def test_mae_learning_rate_schedule_and_config():
    """training/train_mae.py:14-33 (half-cycle cosine after a linear warm-up, in fractional epochs) and the values of
    configs/method/mae/mae.json the MAE route reads."""
    import math
    import os
    from kurosiwo_amd.config import load_json5
    from kurosiwo_amd.training.train_mae import adjust_learning_rate

    class Opt:
        param_groups = [{"lr": 0.0}, {"lr": 0.0, "lr_scale": 0.5}]

    cfg = {"warmup_epochs": 10, "lr": 4e-5, "min_lr": 0.0, "epochs": 100}
    assert adjust_learning_rate(Opt, 0.0, cfg) == 0.0
    assert abs(adjust_learning_rate(Opt, 2.5, cfg) - 1e-5) < 1e-12
    assert Opt.param_groups[1]["lr"] == 0.5 * Opt.param_groups[0]["lr"]
    mid = adjust_learning_rate(Opt, 55.0, cfg)
    assert abs(mid - 4e-5 * 0.5 * (1 + math.cos(math.pi * 45 / 90))) < 1e-12
    assert abs(adjust_learning_rate(Opt, 100.0, cfg)) < 1e-12
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    mc = load_json5(os.path.join(root, "configs/method/mae/mae.json"))
    assert (mc["dim"], mc["depth"], mc["heads"], mc["mlp_dim"], mc["decoder_dim"], mc["decoder_depth"], mc["decoder_heads"]) == (1024, 24, 16, 2048, 512, 8, 16)
    assert mc["masked_ratio"] == 0.75 and mc["accumulate_gradients"] == 4 and mc["warmup_epochs"] == 10


def test_multi_scale_prediction_and_factory_guards():
    """change_detection_trainer.py:139-146: mean of the five outputs, coarse ones nearest-resized; `multi_scale_train` is refused with the
    reason (the reference branch :155-162 raises on the int64 mask), `multi_scale_infer` is accepted."""
    import torch
    from kurosiwo_amd.training.change_detection_trainer import multi_scale_prediction
    g = torch.Generator().manual_seed(3)
    outs = [torch.randn(2, 3, s, s, generator=g) for s in (7, 14, 28, 56, 224)]
    got = multi_scale_prediction(outs)
    want = sum(o.repeat_interleave(224 // o.shape[2], 2).repeat_interleave(224 // o.shape[3], 3) for o in outs) / 5    # nearest at integer factors
    assert got.shape == (2, 3, 224, 224) and torch.allclose(got, want, atol=1e-6)
    with pytest.raises(NotImplementedError, match="Long|int64"):     # what the reference's multi_scale_train line does
        torch.nn.functional.interpolate(torch.zeros(2, 8, 8, dtype=torch.long), size=4, mode="nearest")
    from kurosiwo_amd.model_utilities import initialize_cd_model
    with pytest.raises(NotImplementedError, match="multi_scale_train"):
        initialize_cd_model({"method": "changeformer", "num_channels": 2, "num_classes": 3, "device": "cpu"},
                            {"embed_dim": 256, "decoder_softmax": False, "multi_scale_train": True, "multi_scale_infer": False})


def test_shard_batch_python_lists_and_scalars():
    """per-sample python values (tile names) are cut with the tensors; 0-dim tensors and the per-channel scale lists pass through"""
    import torch
    from kurosiwo_amd.distributed import shard_batch
    x = torch.arange(8 * 3).reshape(8, 3)
    names = [f"tile{i}" for i in range(8)]
    scales = [torch.arange(8.0), torch.arange(8.0) + 10]        # list of per-channel [B] tensors (Dataset.py:844-858)
    flag = torch.tensor(7)
    a = shard_batch((x, names, scales, flag), rank=1, world=4)
    assert a[0].tolist() == x[2:4].tolist() and a[1] == ["tile2", "tile3"]
    assert [t.tolist() for t in a[2]] == [[2.0, 3.0], [12.0, 13.0]] and int(a[3]) == 7


def test_launch_list_orders_side_stream_gradients_behind_tagged_waits(monkeypatch):
    """launch.LaunchList / StepStreams without a GPU: a launch tagged "side" goes to the side stream behind a fork and leaves a mark
    under its side_tag; "@wait_side" entries make the issuing lane wait for exactly that mark (None: for the whole side stream, once);
    without streams every entry runs in list order on the current stream and the waits are no-ops."""
    from kurosiwo_amd import launch as sp
    monkeypatch.setattr(sp, "stream_ptr", lambda: "MAIN")         # (the current HIP stream: no GPU here)

    log = []

    class Lib:
        def ksmi_a(self, x, st):
            log.append(("a", x, st))
            return 0

        def ksmi_w(self, x, st):
            log.append(("w", x, st))
            return 0

    ll = sp.LaunchList()
    ll.add("ksmi_a", lambda: (1,))
    ll.add("ksmi_w", lambda: (2,), {"kind": "wgrad", "bytes": 0, "flops": 0, "side": True, "side_tag": "L0.ff2"})
    ll.add("ksmi_a", lambda: (3,))
    ll.add_wait_side("L0.ff2")
    ll.add_wait_side("never-launched")
    ll.add("ksmi_w", lambda: (4,), {"kind": "wgrad", "bytes": 0, "flops": 0, "side": True})
    ll.add_wait_side(None)
    ll.add_wait_side(None)
    ll.resolve(Lib())
    assert [c[2] for c in ll.calls] == ["ksmi_a", "ksmi_w", "ksmi_a", "@wait_side", "@wait_side", "ksmi_w", "@wait_side", "@wait_side"]
    assert [c[0] is None for c in ll.calls] == [False, False, False, True, True, False, True, True]

    class Streams:                       # the StepStreams surface LaunchList.run uses, recording instead of touching HIP
        lanes, use_side = False, True

        def __init__(self):
            self.ops = []

        def begin(self):
            self.ops.append("begin")

        def fork_side(self, lane, ix=0):
            self.ops.append("fork")
            return "SIDE"

        def mark_side(self, tag, ix=0):
            self.ops.append(("mark", tag))

        def wait_side(self, tag, lane, cur):
            self.ops.append(("wait", tag))

    hooked = []
    ss = Streams()
    ll.run(None, hooked.append, ss)
    assert [(k, x) for k, x, _ in log] == [("a", 1), ("w", 2), ("a", 3), ("w", 4)]
    assert [st for _, _, st in log][1] == "SIDE" and [st for _, _, st in log][3] == "SIDE" and log[0][2] != "SIDE"
    assert ss.ops == ["begin", "fork", ("mark", "L0.ff2"), ("wait", "L0.ff2"), ("wait", "never-launched"), "fork", ("wait", None), ("wait", None)]
    assert hooked == list(range(8))                      # the bucket hook sees every entry, waits included
    del log[:]
    ll.run()                                             # no streams: list order on the current stream
    assert [(k, x) for k, x, _ in log] == [("a", 1), ("w", 2), ("a", 3), ("w", 4)] and all(st != "SIDE" for _, _, st in log)


class _FakeStream:
    """what StepStreams asks of a torch stream, recording instead of touching HIP"""
    def __init__(self, name, log, handle):
        self.name, self.log, self.cuda_stream = name, log, handle

    def wait_stream(self, s):
        self.log.append((self.name, "wait_stream", s.name))


def _step_streams_without_a_gpu(monkeypatch, log):
    """a launch.StepStreams (side stream on, one compute lane) whose streams are recorders; its runner is bound to null streams, so
    nothing of HIP is touched"""
    import ctypes as C
    from kurosiwo_amd import launch as sp
    monkeypatch.setattr(sp, "stream_ptr", lambda: "MAIN")
    main = _FakeStream("main", log, 0)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: main)
    ss = object.__new__(sp.StepStreams)
    ss.side, ss.side2, ss.lane1, ss.side_ptr, ss.side2_ptr = _FakeStream("side", log, 1), None, None, C.c_void_p(None), None
    ss.lanes, ss.use_side, ss.main = False, True, None
    return sp, ss


def test_step_streams_join_reaches_the_runner(monkeypatch):
    """StepStreams.join() is ksmi_runner_join exactly when a runner exists (the step's stream state has one owner), and a current
    stream other than main then waits for main; end() = join() + reset"""
    from kurosiwo_amd import _lib
    log, joined = [], []
    sp, ss = _step_streams_without_a_gpu(monkeypatch, log)
    lib = _lib.load()
    real = lib.ksmi_runner_join
    monkeypatch.setattr(lib, "ksmi_runner_join", lambda r: joined.append(r.value) or real(r))
    ss.join()
    assert joined == [] and log == []                  # nothing ran on these streams: no runner, nothing to wait for
    ss.begin()
    r = ss.runner()
    assert r.value and ss._runner is r
    ss.join()
    assert joined == [r.value] and log == []           # the caller is on main: the runner's join is all of it
    other = _FakeStream("other", log, 2)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: other)
    ss.join()
    assert joined == [r.value, r.value] and log == [("other", "wait_stream", "main")]
    ss.end()
    assert joined == [r.value] * 3 and log == [("other", "wait_stream", "main")] * 2 and ss.main is None
    ss.join()                                          # between steps: the runner's (empty) join, no stream to wait for
    assert joined == [r.value] * 4 and len(log) == 2


def test_mirror_freshness_and_skip_if_without_a_gpu(monkeypatch):
    """The bf16 operand copy of the parameters (plan_base.wb): the optimiser that wrote it marks it with the version counter of the
    fp32 arena; the cast launch of the NEXT forward is skipped iff no in-place torch operation touched a parameter since, and the mark
    is consumed by that one forward.  LaunchList honours meta["skip_if"].  conv_npad: 32 padded columns for the thin heads."""
    import torch
    from kurosiwo_amd import launch as sp, plan_base as pb
    from kurosiwo_amd.runtime import conv_npad
    assert [conv_npad(n) for n in (1, 2, 3, 15, 16, 17, 32, 48, 100)] == [32, 32, 32, 32, 16, 32, 32, 48, 112]

    class M:
        flat_params = torch.zeros(64)

    class P(pb.PlanBase):
        def __init__(self):
            self.m, self.wb = M(), torch.zeros(64, dtype=torch.bfloat16)
            self._mirror_version = None

    p = P()
    assert p._mirror_is_fresh() is False                         # nobody wrote the mirror: cast
    p.mirror_written()
    assert p._mirror_is_fresh() is True and p._mirror_is_fresh() is False      # consumed by one forward
    p.mirror_written()
    view = p.m.flat_params[8:16]
    with torch.no_grad():
        view.mul_(2.0)                                           # load_state_dict / init: an in-place op on a view of the arena
    assert p._mirror_is_fresh() is False
    # two cached plans of ONE model (a batch-shape change rebuilds the train step, the plans stay in model._plans): the optimiser writes
    # the parameters through raw pointers, which torch's version counter never sees -- the arena generation every fused step bumps
    # does (plan A must cast again after plan B stepped, or it runs one optimiser step stale)
    from kurosiwo_amd import optim
    a, b = P(), P()
    b.m = a.m                                                    # the same arena
    optim._bump_generation(a.m.flat_params.data_ptr()); a.mirror_written()          # step on A (mirrored)
    assert a._mirror_is_fresh() is True
    optim._bump_generation(a.m.flat_params.data_ptr()); a.mirror_written()          # step on A again ...
    optim._bump_generation(a.m.flat_params.data_ptr()); b.mirror_written()          # ... then a step on B: only wb_B was written
    assert a._mirror_is_fresh() is False and b._mirror_is_fresh() is True
    optim._bump_generation(a.m.flat_params.data_ptr()); a.mirror_written()          # an UNMIRRORED step of anything else afterwards (SGD, the autograd path)
    optim._bump_generation(a.m.flat_params.data_ptr())
    assert a._mirror_is_fresh() is False
    monkeypatch.setenv("KSMI_ADAM_MIRROR", "0")
    assert p.mirror_ptr() is None
    monkeypatch.delenv("KSMI_ADAM_MIRROR")
    assert p.mirror_ptr() == p.wb.data_ptr()
    p._mirror_off = True                                         # (graph capture: the replay cannot re-decide)
    assert p.mirror_ptr() is None

    monkeypatch.setattr(sp, "stream_ptr", lambda: "MAIN")
    log, fresh = [], [False]

    class Lib:
        def ksmi_cast(self, st):
            log.append("cast")
            return 0

        def ksmi_fwd(self, st):
            log.append("fwd")
            return 0

    ll = sp.LaunchList()
    ll.add("ksmi_cast", lambda: (), {"kind": "cast_bf16", "bytes": 0, "flops": 0, "skip_if": lambda: fresh[0]})
    ll.add("ksmi_fwd", lambda: ())
    ll.resolve(Lib())
    ll.run()
    fresh[0] = True
    ll.run()
    assert log == ["cast", "fwd", "fwd"]


def test_bf16_storage_emulation_contract(golden_dir):
    """oracle/bf16_storage.py (test infrastructure behind tests/golden/snunet_parity_draws_ref.npz and snunet_dem_shard_bf16emu.npz):
    stored tensors and the gradients arriving at them are bf16 values, convolution weights are bf16 operands with an fp32 master
    gradient, modules named in `skip` stay fp32; and the two fixtures carry what the GPU gates read."""
    import numpy as np
    from oracle import bf16_storage as S

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.conv = torch.nn.Conv2d(3, 4, 3, padding=1)
            self.act = torch.nn.ReLU()
            self.head = torch.nn.Conv2d(4, 2, 1)

        def forward(self, x):
            return self.head(self.act(self.conv(x)))

    torch.manual_seed(0)
    net = Net()
    seen = {}
    net.act.register_forward_hook(lambda m, i, o: seen.__setitem__("act", o))
    patched = S.attach(net, skip=("head",), fp32_operands=())
    assert patched == ["conv", "act"]
    x = torch.randn(2, 3, 8, 8, requires_grad=True)
    y = net(x)
    is_bf16 = lambda t: torch.equal(t, t.to(torch.bfloat16).float())
    assert is_bf16(seen["act"].detach()) and not is_bf16(y.detach())       # stored activation rounded, fp32 head output not
    g = torch.randn_like(y)
    y.backward(g)
    assert is_bf16(x.grad)                                                  # gradient rounded where it is stored
    assert not is_bf16(net.conv.weight.grad)                                # master-weight gradient stays fp32
    # forward value = convolution of the ROUNDED operands
    ref = torch.nn.functional.conv2d(S.bf16_round(x.detach()), S.bf16_round(net.conv.weight.detach()), net.conv.bias.detach(), padding=1)
    assert torch.equal(seen["act"].detach(), S.bf16_round(torch.relu(S.bf16_round(ref))))
    d = np.load(os.path.join(golden_dir, "snunet_parity_draws_ref.npz"))
    assert d["bf16emu.miou40"].shape == (23,) and d["fp32.miou40"].shape == (4,) and d["bf16emu.losses"].shape == (23, 40)
    e = np.load(os.path.join(golden_dir, "snunet_dem_shard_bf16emu.npz"))
    f = np.load(os.path.join(golden_dir, "snunet_dem_shard.npz"))
    r = e["gstat.conv0_0.conv1.weight"]
    assert abs(r[1] - f["gstat.conv0_0.conv1.weight"][0]) < 1e-3 * r[1]     # its fp32 column is the fp32 fixture's
    assert 0.90 < r[0] / r[1] < 0.95                                        # bf16 storage lowers the first block's gradient norm by 5-9 % on the reference itself
