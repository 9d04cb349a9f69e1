"""The augmentation-view kernels (csrc/augment.hip: ksmi_augment_views, ksmi_augment_masks) against the float64 oracle
tests/augment_ref.py, against ksmi_sar_preprocess (identity rows: bit-identical), and the loaders that feed them (SSLBatchLoader,
TileBatchLoader(augment=...), train_mae.train, prepare_loaders) on a synthetic archive."""
import gzip
import os
import pickle
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "tools"))

import augment_ref as R                                              # noqa: E402
from test_dataset_cpu import MEAN, STD, TEST, TRAIN, VAL, _configs            # noqa: E402

DEV = "cuda"
IDENT = [0, 0, 224, 224, 0, 0]


def _dev(a, dtype=None):
    return torch.as_tensor(a, dtype=dtype).to(DEV).contiguous()


@pytest.mark.parametrize("C", [1, 2, 3, 6])
def test_kernel_matches_the_float64_oracle(C):
    from kurosiwo_amd import augment as A
    B = 8
    raw, rows = R.raw_tiles(20 + C, B, C), R.boxes(7, B)
    assert np.isnan(raw).any() and (raw < 0).any() and (raw > 0.15).any()
    assert {tuple(r[4:]) for r in rows.tolist()} == {(0, 0), (1, 0), (0, 1), (1, 1)}
    mean, std = (MEAN * 3)[:C], (STD * 3)[:C]
    got = A.apply(_dev(raw), _dev(rows), mean, std, 0.15).cpu().numpy()
    ref = R.views_ref(raw, rows, mean, std, 0.15)
    err = float(np.abs(got - ref).max())
    print(f"C={C}: kernel vs oracle max abs err {err:.3e}, tolerance {R.tolerance(ref):.3e}")
    assert np.isfinite(got).all() and err <= R.tolerance(ref)
    assert np.array_equal(got, A.apply_cpu(raw, rows, mean, std, 0.15))            # the host restatement gives the kernel's bits
    # nearest-mode labels: bit-equal, int64 and uint8; the counts are those of the views
    rng = np.random.default_rng(C)
    for dtype in (np.int64, np.uint8):
        lab = rng.integers(0, 4, (B, 224, 224)).astype(dtype)
        view, count = A.apply_masks(_dev(lab), _dev(rows), count=True)
        want = np.stack([R.mask_ref(lab[b], rows[b]) for b in range(B)])
        assert view.dtype == _dev(lab).dtype and np.array_equal(view.cpu().numpy(), want)
        assert count.cpu().tolist() == [int((w != 0).sum()) for w in want]


@pytest.mark.parametrize("clamp", [0.15, -1.0])
def test_identity_rows_are_bit_identical_to_sar_preprocess(clamp):
    from kurosiwo_amd import augment as A
    from kurosiwo_amd.data import preprocess_gpu
    raw = R.raw_tiles(3, 4, 6)
    raw[0, 0, 0, :8] = -0.0
    x = _dev(raw)
    rows = _dev(np.tile(np.array(IDENT, np.int32), (4, 1)))
    old = preprocess_gpu(x, MEAN * 3, STD * 3, clamp)
    new = A.apply(x, rows, MEAN * 3, STD * 3, clamp)
    assert torch.equal(old.view(torch.int32), new.view(torch.int32))
    assert bool(torch.isnan(new).any()) == (clamp < 0)


def test_supervised_fallback_on_the_device():
    """boxes over a no-data corner: the samples whose augmented valid mask is empty come back un-augmented (image and label), the
    others augmented, decided by the device word"""
    from kurosiwo_amd import augment as A
    B = 6
    raw = R.raw_tiles(9, B, 2)
    valid = np.ones((B, 224, 224), np.float32)
    valid[:, :64, :64] = 0                                                   # the no-data corner
    lab = np.random.default_rng(1).integers(0, 3, (B, 224, 224)).astype(np.int64)
    rows = np.array([[0, 0, 64, 64, 0, 0], [10, 10, 40, 50, 1, 0], [0, 0, 65, 64, 0, 0], [100, 100, 50, 60, 1, 0], [5, 20, 30, 30, 0, 1],
                     [0, 32, 64, 64, 1, 1]], np.int32)
    x, t = _dev(raw), _dev(rows)
    _, alive = A.apply_masks(_dev(valid), t, count=True, write=False)
    empty = alive.cpu().numpy() == 0
    assert empty.tolist() == [True, True, False, False, True, False] and empty.any() and (~empty).any()         # both branches occur
    img = A.apply(x, t, MEAN, STD, 0.15, fallback=alive).cpu().numpy()
    lbl, _ = A.apply_masks(_dev(lab), t, fallback=alive)
    ident = np.tile(np.array(IDENT, np.int32), (B, 1))
    plain = A.apply_cpu(raw, ident, MEAN, STD, 0.15)
    augmented = A.apply_cpu(raw, rows, MEAN, STD, 0.15)
    for b in range(B):
        if empty[b]:
            assert np.array_equal(img[b], plain[b]) and np.array_equal(lbl[b].cpu().numpy(), lab[b])
        else:
            assert np.array_equal(img[b], augmented[b]) and not np.array_equal(img[b], plain[b])
            assert np.array_equal(lbl[b].cpu().numpy(), R.mask_ref(lab[b], rows[b]))


def test_noise_and_dropout_ops():
    from kurosiwo_amd import augment as A
    raw = R.raw_tiles(2, 4, 3)
    rows = np.tile(np.array(IDENT, np.int32), (4, 1))
    rows[1] = (20, 30, 100, 120, 1, 0)
    x, t = _dev(raw), _dev(rows)
    mean, std = [0.0] * 3, [1.0] * 3
    state = lambda seed, step: _dev(np.array([seed, step], np.int32))
    pipe = A.build_pipeline({"MultNoise": {"p": 1.0}, "GaussianNoise": {"p": 1.0, "var_limit": [1e-4, 4e-4]}, "Cutout": {"p": 1.0}})
    plain = A.apply(x, t, mean, std, 0.15).cpu().numpy()
    a = A.apply(x, t, mean, std, 0.15, pipe, rng_state=state(7, 3)).cpu().numpy()
    assert np.array_equal(a, A.apply(x, t, mean, std, 0.15, pipe, rng_state=state(7, 3)).cpu().numpy())          # repeatable
    nxt = A.apply(x, t, mean, std, 0.15, pipe, rng_state=state(7, 4)).cpu().numpy()
    assert not np.array_equal(a, nxt) and not np.array_equal(a == 0, nxt == 0)                                    # step + 1 differs
    holes = a == 0
    assert holes.any() and np.array_equal(holes[:, 0], holes[:, 1]) and np.array_equal(holes[:, 0], holes[:, 2])   # the same in every channel
    assert all(0 < holes[b, 0].sum() <= 8 * 64 for b in range(4))
    resid = (a - plain)[~holes]
    assert 0.005 < resid.std() < 0.03 and abs(resid.mean()) < 2e-3
    # the integer-driven ops give the host restatement's bits; the Gaussian one agrees to the rounding of logf / cosf
    exact = A.build_pipeline({"Cutout": {"p": 1.0, "max_holes": 5, "max_height": 16, "max_width": 12}, "MultNoise": {"p": 0.5}})
    got = A.apply(x, t, mean, std, 0.15, exact, rng_state=state(11, 2)).cpu().numpy()
    assert np.array_equal(got, A.apply_cpu(raw, rows, mean, std, 0.15, exact, rng_words=(11, 2)))
    host = A.apply_cpu(raw, rows, mean, std, 0.15, pipe, rng_words=(7, 3))
    assert np.array_equal(host == 0, holes) and float(np.abs(host - a).max()) < 1e-5
    # p = 0: the identity, and no rng state is needed
    off = A.build_pipeline({"MultNoise": {"p": 0.0}, "GaussianNoise": {"p": 0.0}, "Cutout": {"p": 0.0}})
    assert np.array_equal(A.apply(x, t, mean, std, 0.15, off).cpu().numpy(), plain)
    with pytest.raises(ValueError):
        A.apply(x, t, mean, std, 0.15, pipe)


# ---- loaders end to end --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def archive(tmp_path_factory):
    from make_synthetic_archive import make
    root = str(tmp_path_factory.mktemp("ks"))
    os.makedirs(os.path.join(root, "pickle"))
    tr, truth = make(root, TRAIN, tiles_per_act=4, seed=1)
    te, _ = make(root, VAL + TEST, tiles_per_act=4, seed=2)
    pickle.dump(tr, gzip.open(os.path.join(root, "pickle", "train.gz"), "wb"))
    pickle.dump(te, gzip.open(os.path.join(root, "pickle", "test.gz"), "wb"))
    return root, truth


def test_ssl_loader_equals_the_host_path(archive, tmp_path):
    from kurosiwo_amd import augment as A
    from kurosiwo_amd import geotiff
    from kurosiwo_amd.dataset import SSLBatchLoader, SSLDataset
    root, _ = archive
    ds = SSLDataset(_configs(root), cache=str(tmp_path / "ssl.pkl"))
    assert len(ds) == 16
    mk = lambda **kw: SSLBatchLoader(ds, 8, shuffle=True, drop_last=True, device=DEV, threads=4, seed=5, **kw)
    one = mk(prefetch=0)
    order = list(one._index_lists())
    one = mk(prefetch=0)
    batches = []
    for idx in order:
        (img,) = one.load(idx)
        assert img.is_cuda and img.shape == (8, 6, 224, 224) and img.dtype == torch.float32
        rows = one.last_params
        raw = np.stack([np.stack([geotiff.read(p, dtype=np.float32)[0] for p in ds.sample_paths(i)]) for i in idx])
        want = A.apply_cpu(raw, rows, MEAN * 3, STD * 3, 0.15)
        ref = R.views_ref(raw, rows, MEAN * 3, STD * 3, 0.15)
        assert float(np.abs(img.cpu().numpy() - ref).max()) <= R.tolerance(ref)
        assert np.array_equal(img.cpu().numpy(), want)
        batches.append(img.cpu())
    assert len(batches) == 2 and sorted(sum((list(i) for i in order), [])) == list(range(16))
    again = [b[0].cpu() for b in mk()]                                     # the prefetching iterator, same seed: the same views
    assert len(again) == 2 and all(torch.equal(a, b) for a, b in zip(again, batches))
    parts = [[b[0].cpu() for b in mk(rank=r, world=2)] for r in (0, 1)]     # two ranks' slices concatenate to the one-rank batch
    for b in range(2):
        assert parts[0][b].shape[0] == 4 and torch.equal(torch.cat((parts[0][b], parts[1][b])), batches[b])


def test_train_mae_runs_from_the_archive(archive, tmp_path, monkeypatch):
    from kurosiwo_amd.config import load_json5
    from kurosiwo_amd.training import train_mae
    import kurosiwo_amd.dataset as DS
    root, _ = archive
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    monkeypatch.setenv("KSMI_DATA", "archive")
    monkeypatch.chdir(tmp_path)
    seen = {"batches": 0}
    orig = DS.SSLBatchLoader._load

    def spy(self, idx):
        seen["batches"] += 1
        return orig(self, idx)
    monkeypatch.setattr(DS.SSLBatchLoader, "_load", spy)
    logs = []
    orig_epoch = train_mae.train_epoch

    def keep(*a, **kw):
        out = orig_epoch(*a, **kw)
        logs.extend(out)
        return out
    monkeypatch.setattr(train_mae, "train_epoch", keep)
    cfg = load_json5(os.path.join(repo, "configs", "method", "mae", "mae.json"))
    cfg.update(_configs(root, device="cuda:0"))
    cfg.update(batch_size=8, num_samples_per_epoch=32, epochs=2, warmup_epochs=0, learning_rate=1e-4, min_lr=1e-5, accumulate_gradients=None,
               checkpoint_path=str(tmp_path / "ck"), num_channels=2, seed=3, depth=2, mlp_dim=256, decoder_depth=1)
    model = train_mae.train(cfg, precision="bf16")
    assert seen["batches"] >= 8 and cfg["num_channels"] == 6 and model.hp["channels"] == 6
    losses = [l["train loss"] for l in logs]
    print("MAE losses from the archive:", losses)
    assert len(losses) == 2 and all(np.isfinite(losses)) and losses[-1] < losses[0]
    assert os.path.isfile(tmp_path / "ck" / "ssl_samples.pkl") and os.path.isfile(tmp_path / "ck" / "mae_vit_2.pt")
    assert not os.path.exists(tmp_path / "ssl_samples.pkl")


def test_prepare_loaders_with_data_augmentations(archive, monkeypatch):
    from kurosiwo_amd import augment as A
    from kurosiwo_amd.data import prepare_loaders
    from kurosiwo_amd.dataset import Dataset, TileBatchLoader
    root, truth = archive
    monkeypatch.setenv("KSMI_DATA", "archive")
    cfg = _configs(root, device=DEV, data_augmentations=True, batch_size=4, dem=True, seed=2)
    tr, va, te = prepare_loaders(cfg)
    assert isinstance(tr, TileBatchLoader) and tr.augment is not None and va.augment is None and te.augment is None
    assert cfg["data_augmentations"] is True and list(cfg["augmentations"])[0] == "RandomResizedCrop"
    plain_val = next(iter(TileBatchLoader(Dataset("val", _configs(root, device=DEV, dem=True)), 4, device=DEV)))
    assert all(torch.equal(a, b) for a, b in zip(next(iter(va)), plain_val) if torch.is_tensor(a))        # val is untouched
    ds = tr.ds
    n_aug = n_plain = nbatches = 0
    for idx in tr._index_lists():
        nbatches += 1
        batch = tr.load(idx)
        rows = tr.last_params
        assert len(batch) == 13 and batch[2].shape == (4, 2, 224, 224) and batch[3].dtype == torch.int64 and batch[10].shape == (4, 1, 224, 224)
        ident = np.tile(np.array(IDENT, np.int32), (4, 1))
        for j, i in enumerate(idx):
            t = truth[ds.records[i]["id"]]
            _, alive = A.apply_masks_cpu(t["valid"][None], rows[j:j + 1])
            row = rows[j:j + 1] if alive[0] else ident[:1]
            n_aug += int(alive[0] > 0 and not np.array_equal(row[0], IDENT))
            n_plain += int(alive[0] == 0)
            for pos, key in ((2, "MS1"), (6, "SL1"), (9, "SL2")):
                ref = R.view_ref(t[key], row[0], MEAN, STD, 0.15)
                assert float(np.abs(batch[pos][j].cpu().numpy() - ref).max()) <= R.tolerance(ref)
            assert np.array_equal(batch[3][j].cpu().numpy(), R.mask_ref(t["mask"].astype(np.int64), row[0]))
            assert torch.equal(batch[10][j].cpu(), ds[i][10])                       # the DEM is not augmented (as in the reference)
            assert int(batch[12][j]) == t["act"]
    assert nbatches == 2 and n_aug >= 4
    # where the batch-level loader is not eligible, the flag raises as it always did
    with pytest.raises(NotImplementedError):
        prepare_loaders(_configs(root, device=DEV, data_augmentations=True, batch_size=4, gpu_input_pipeline=False))
    with pytest.raises(NotImplementedError):
        TileBatchLoader(Dataset("val", _configs(root, device=DEV)), 4, device=DEV, augment=tr.augment)
