"""Augmentation views on the host (kurosiwo_amd/augment.py) and SSLDataset (kurosiwo_amd/dataset.py) against the float64 oracle
tests/augment_ref.py and the reference's own expressions on a synthetic archive.  cv2 / albumentations are in no image of this
project, so the resize is formula-pinned (see the header of csrc/augment.hip) -- like the losses."""
import math
import os
import pickle
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "tools"))

import augment_ref as R                                              # noqa: E402
from test_dataset_cpu import MEAN, STD, TRAIN, _configs, _ref_concat, _ref_normalize          # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the oracle itself ------------------------------------------------------------------------------------------------------------------
def test_oracle_is_self_consistent():
    rng = np.random.default_rng(0)
    img = rng.random((2, 224, 224))
    assert np.array_equal(R.resize_ref(img), img)                                        # 224 x 224: the identity
    half = rng.random((2, 112, 112))
    assert np.array_equal(R.resize_ref(half), half.repeat(2, axis=1).repeat(2, axis=2))  # 112 x 112: exact 2 x replication
    assert np.array_equal(R.resize_ref(np.full((1, 37, 91), 0.125)), np.full((1, 224, 224), 0.125))      # a constant stays constant
    for n in range(1, 225):
        taps = R.area_taps(n)
        assert all(0.0 <= f < 1.0 and 0 <= s <= sb <= n - 1 and sb - s <= 1 for s, sb, f in taps), n
        assert [s for s, _, _ in taps] == sorted(s for s, _, _ in taps) and taps[0][0] == 0
        assert all(0 <= s <= n - 1 for s in R.nearest_taps(n))
    assert R.nearest_taps(224) == list(range(224)) and R.nearest_taps(112) == [d // 2 for d in range(224)]
    row = (3, 5, 100, 60, 1, 1)
    m = rng.integers(0, 4, (224, 224))
    flipped, plain = R.mask_ref(m, row), R.mask_ref(m, (3, 5, 100, 60, 0, 0))
    assert np.array_equal(flipped, plain[::-1, ::-1])


# ---- apply_cpu against the oracle ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 2, 6])
def test_apply_cpu_matches_the_oracle(C):
    from kurosiwo_amd import augment as A
    raw, rows = R.raw_tiles(10 + C, 9, C), R.boxes(3, 9)
    mean, std = (MEAN * 3)[:C], (STD * 3)[:C]
    got = A.apply_cpu(raw, rows, mean, std, 0.15)
    ref = R.views_ref(raw, rows, mean, std, 0.15)
    assert got.dtype == np.float32 and np.isfinite(got).all()
    err = float(np.abs(got - ref).max())
    print("apply_cpu vs oracle: max abs err", err, "tolerance", R.tolerance(ref))
    assert err <= R.tolerance(ref)
    # index choices are integer arithmetic: exact
    for n in (1, 2, 77, 112, 223, 224):
        s, sb, f = A.area_coefficients(n)
        assert [(int(a), int(b)) for a, b in zip(s, sb)] == [(a, b) for a, b, _ in R.area_taps(n)]
        assert np.array_equal(f, np.array([w for _, _, w in R.area_taps(n)]).astype(np.float32)) and f.dtype == np.float32
        assert A.nearest_indices(n).tolist() == R.nearest_taps(n)
    # identity rows: the Dataset's clamp -> nan_to_num -> Normalize, bit for bit (-0 and NaN neighbours included)
    ident = np.tile(np.array([0, 0, 224, 224, 0, 0], np.int32), (9, 1))
    want = torch.stack([_ref_normalize(torch.nan_to_num(torch.clamp(torch.from_numpy(t), 0.0, 0.15), 0.15), mean, std) for t in raw])
    assert torch.equal(A.apply_cpu(torch.from_numpy(raw), ident, mean, std, 0.15), want)
    # no clamp (SLC-style): NaN taps stay NaN and do not leak through zero coefficients
    got = A.apply_cpu(raw, ident, mean, std, None)
    assert np.array_equal(np.isnan(got), np.isnan(raw))
    # the fallback word: 0 -> identity for that sample only
    fb = np.array([1, 0, 1, 0, 5, 1, 1, 1, 1], np.int32)
    got = A.apply_cpu(raw, rows, mean, std, 0.15, fallback=fb)
    assert np.array_equal(got[fb == 0], want.numpy()[fb == 0]) and np.array_equal(got[fb != 0], A.apply_cpu(raw, rows, mean, std, 0.15)[fb != 0])


def test_label_views_are_bit_equal():
    from kurosiwo_amd import augment as A
    rng = np.random.default_rng(5)
    rows = R.boxes(4, 9)
    for dtype in (np.int64, np.uint8):
        lab = rng.integers(0, 4, (9, 224, 224)).astype(dtype)
        got, count = A.apply_masks_cpu(lab, rows)
        want = np.stack([R.mask_ref(lab[b], rows[b]) for b in range(9)])
        assert got.dtype == dtype and np.array_equal(got, want)
        assert count.tolist() == [int((w != 0).sum()) for w in want]
    got, _ = A.apply_masks_cpu(torch.from_numpy(lab), rows, fallback=np.array([0] * 9))
    assert torch.equal(got, torch.from_numpy(lab))


def test_noise_and_dropout_ops_on_the_host():
    from kurosiwo_amd import augment as A
    raw = R.raw_tiles(2, 4, 3)
    rows = np.tile(np.array([0, 0, 224, 224, 0, 0], np.int32), (4, 1))
    mean, std = [0.0] * 3, [1.0] * 3
    plain = A.apply_cpu(raw, rows, mean, std, 0.15)
    pipe = A.build_pipeline({"MultNoise": {"p": 1.0}, "GaussianNoise": {"p": 1.0, "var_limit": [1e-4, 4e-4]}, "Cutout": {"p": 1.0}})
    assert [o[0] for o in pipe.pixel_ops] == [A.OP_MULT, A.OP_GAUSS, A.OP_CUT] and pipe.kernel_args()[-1] == 1 | 2 << 2 | 3 << 4
    a = A.apply_cpu(raw, rows, mean, std, 0.15, pipe, rng_words=(7, 3))
    assert np.array_equal(a, A.apply_cpu(raw, rows, mean, std, 0.15, pipe, rng_words=(7, 3)))
    assert not np.array_equal(a, A.apply_cpu(raw, rows, mean, std, 0.15, pipe, rng_words=(7, 4)))
    holes = a == 0
    assert holes.any() and np.array_equal(holes[:, 0], holes[:, 1]) and np.array_equal(holes[:, 0], holes[:, 2])
    assert all(0 < holes[b, 0].sum() <= 8 * 64 for b in range(4))
    resid = (a - plain)[~holes]
    assert 0.005 < resid.std() < 0.03                                     # sigma in [0.01, 0.02] + a factor in [0.9, 1.1) on values <= 0.15
    off = A.build_pipeline({"MultNoise": {"p": 0.0}, "GaussianNoise": {"p": 0.0}, "Cutout": {"p": 0.0}})
    assert off.pixel_ops == () and np.array_equal(A.apply_cpu(raw, rows, mean, std, 0.15, off), plain)
    only = A.build_pipeline({"MultNoise": {"p": 1.0, "multiplier": [0.5, 0.75]}})
    r = A.apply_cpu(raw, rows, mean, std, 0.15, only, rng_words=(1, 1)) / np.where(plain == 0, 1, plain)
    for b in range(4):
        f = r[b][plain[b] != 0]
        assert 0.5 <= f.min() and f.max() < 0.75 + 1e-6 and f.max() - f.min() < 1e-6      # one factor per sample
    with pytest.raises(ValueError):
        A.apply_cpu(raw, rows, mean, std, 0.15, pipe)


# ---- sample_resized_crop -------------------------------------------------------------------------------------------------------------------
def _analytic_mean_area(scale, ratio, H, W, grid=1500):
    """mean covered-area fraction of the accept-or-fallback process by enumeration (midpoint rule over the two uniform draws of an
    attempt, float64); ten attempts, then the centred fallback"""
    u = scale[0] + (scale[1] - scale[0]) * (np.arange(grid) + 0.5) / grid
    la = math.log(ratio[0]) + (math.log(ratio[1]) - math.log(ratio[0])) * (np.arange(grid) + 0.5) / grid
    area, asp = np.meshgrid(u * H * W, np.exp(la), indexing="ij")
    w, h = np.rint(np.sqrt(area * asp)), np.rint(np.sqrt(area / asp))
    ok = (w > 0) & (w <= W) & (h > 0) & (h <= H)
    p = ok.mean()
    inside = (w * h / (H * W))[ok].mean()
    in_ratio = W / H
    if in_ratio < min(ratio):
        fw, fh = W, round(W / min(ratio))
    elif in_ratio > max(ratio):
        fh, fw = H, round(H * max(ratio))
    else:
        fw, fh = W, H
    miss = (1 - p) ** 10
    return (1 - miss) * inside + miss * fw * fh / (H * W)


def test_sample_resized_crop():
    from kurosiwo_amd.augment import sample_resized_crop
    a = [sample_resized_crop(random.Random(5), 224, 224, (0.2, 1.0)) for _ in range(3)]
    assert a[0] == a[1] == a[2]
    rng = random.Random(11)
    boxes = [sample_resized_crop(rng, 224, 224, (0.2, 1.0)) for _ in range(20000)]
    assert all(0 <= y0 and 0 <= x0 and 0 < h and 0 < w and y0 + h <= 224 and x0 + w <= 224 for y0, x0, h, w in boxes)
    got = float(np.mean([h * w / 224 ** 2 for _, _, h, w in boxes]))
    want = _analytic_mean_area((0.2, 1.0), (3 / 4, 4 / 3), 224, 224)
    print("mean area fraction", got, "analytic", want)
    assert abs(got - want) <= 0.01
    assert len({b[:2] for b in boxes}) > 1000                                 # the corner moves
    # the fallback: no attempt can fit, the centred crop clamped by the ratio comes back without a corner draw
    rng = random.Random(1)
    assert sample_resized_crop(rng, 224, 224, (0.9, 1.0), ratio=(3.0, 4.0)) == ((224 - 75) // 2, 0, 75, 224)       # 224 / 3 -> 75 rows
    assert sample_resized_crop(rng, 224, 224, (0.9, 1.0), ratio=(0.2, 0.25)) == (0, (224 - 56) // 2, 224, 56)      # 224 * 0.25 columns
    y0, x0, h, w = sample_resized_crop(random.Random(2), 100, 224, (4.0, 5.0))                                        # in_ratio 2.24 > 4/3
    assert (h, w) == (100, 133) and (y0, x0) == (0, (224 - 133) // 2)


# ---- build_pipeline -------------------------------------------------------------------------------------------------------------------------
def test_build_pipeline_on_the_shipped_json():
    from kurosiwo_amd import augment as A
    from kurosiwo_amd.config import load_json5
    from kurosiwo_amd.data import load_augmentation_config
    shipped = load_json5(os.path.join(ROOT, "configs", "augmentations", "augmentation.json"))
    assert shipped == load_json5(os.path.join(ROOT, "tests", "golden", "reference_configs", "augmentations", "augmentation.json"))
    assert load_augmentation_config({}) == shipped
    assert list(shipped["augmentations"]) == ["RandomResizedCrop", "GaussianBlur", "HorizontalFlip", "VerticalFlip", "ElasticTransform",
                                              "MultNoise", "ColorJitter", "Cutout"]
    pipe = A.build_pipeline(shipped["augmentations"])
    assert pipe.crop == (1.0, (0.2, 1.0), (3 / 4, 4 / 3)) and pipe.hflip == 0.5 and pipe.vflip == 0.0 and pipe.pixel_ops == ()
    assert pipe.kernel_args()[-1] == 0
    rows = pipe.sample_params(random.Random(3), 400)
    assert rows.dtype == np.int32 and rows.shape == (400, 6) and 120 < rows[:, 4].sum() < 280 and rows[:, 5].sum() == 0
    assert np.array_equal(rows, pipe.sample_params(random.Random(3), 400))
    with pytest.raises(KeyError):
        A.build_pipeline(dict(shipped["augmentations"], Posterize={"p": 1.0}))
    for name in ("GaussianBlur", "ElasticTransform"):
        with pytest.raises(NotImplementedError, match=name):
            A.build_pipeline({name: dict(shipped["augmentations"][name], p=0.3)})
    # json order = op order
    swapped = A.build_pipeline({"Cutout": {"p": 0.5}, "MultNoise": {"p": 0.25}})
    assert [o[0] for o in swapped.pixel_ops] == [A.OP_CUT, A.OP_MULT] and swapped.kernel_args()[-1] == 3 | 1 << 2
    with pytest.raises(NotImplementedError):
        A.build_pipeline({"MultNoise": {"p": 0.25}, "RandomResizedCrop": shipped["augmentations"]["RandomResizedCrop"]})


# ---- SSLDataset on a synthetic archive ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def archive(tmp_path_factory):
    from make_synthetic_archive import make
    root = str(tmp_path_factory.mktemp("ssl"))
    _, truth = make(root, TRAIN, tiles_per_act=3, seed=1)
    open(os.path.join(root, "data", str(TRAIN[0]), "aoi.gpkg"), "w").write("")          # skipped by the walk
    return root, truth


def test_ssl_dataset_follows_the_reference(archive, tmp_path, monkeypatch):
    from kurosiwo_amd.dataset import SSLDataset
    root, truth = archive
    monkeypatch.chdir(tmp_path)
    cache = str(tmp_path / "where" / "it" / "was" / "told.pkl")
    ds = SSLDataset(_configs(root), cache=cache)
    want = sorted(os.path.join(root, "data", str(act), aoi, h) for act in TRAIN for aoi in os.listdir(os.path.join(root, "data", str(act)))
                  if ".gpkg" not in aoi for h in os.listdir(os.path.join(root, "data", str(act), aoi)))
    assert len(want) == 6 and pickle.load(open(cache, "rb")) == want
    random.Random(999).shuffle(want)
    assert ds.samples == want and len(ds) == 6
    assert os.listdir(tmp_path) == ["where"]                                   # nothing lands in the working directory
    ck = tmp_path / "ck"
    ds2 = SSLDataset(_configs(root, checkpoint_path=str(ck)))
    assert os.path.isfile(ck / "ssl_samples.pkl") and ds2.samples == want
    assert SSLDataset(_configs(root, checkpoint_path=str(ck))).samples == want        # read back from the cache
    with pytest.raises(ValueError):
        SSLDataset(_configs(root))
    mean3, std3 = MEAN * 3, STD * 3
    views = []
    for i in range(len(ds)):
        image, flood, pre1, pre2 = ds[i]
        t = truth[os.path.basename(ds.samples[i])]
        assert image.shape == (6, 224, 224) and image.dtype == torch.float32 and torch.isfinite(image).all()
        for got, key in ((flood, "MS1"), (pre1, "SL1"), (pre2, "SL2")):
            assert got.shape == (2, 224, 224)
            assert torch.equal(got, _ref_normalize(_ref_concat(t[key][0], t[key][1], ["vv", "vh"], 0.15), MEAN, STD))
        views.append(image)
    # the view is the oracle's view of the six raw channels (flood, pre1, pre2) under the rows the dataset's seeded stream draws
    replay = SSLDataset(_configs(root), cache=cache)
    rows = replay.pipeline.sample_params(random.Random(999), 6)                # configs carry no seed: 999
    for i in range(len(ds)):
        t = truth[os.path.basename(ds.samples[i])]
        raw = np.concatenate([t["MS1"], t["SL1"], t["SL2"]])
        ref = R.view_ref(raw, rows[i], mean3, std3, 0.15)
        assert float(np.abs(views[i].numpy() - ref).max()) <= R.tolerance(ref)
    assert len({tuple(r) for r in rows.tolist()}) == 6


def test_per_sample_dataset_still_has_no_augmented_path(archive):
    from kurosiwo_amd.dataset import Dataset
    root, _ = archive
    with pytest.raises(NotImplementedError):
        Dataset("train", _configs(root, data_augmentations=True))
    with pytest.raises(NotImplementedError):
        Dataset("train", _configs(root, task="self-supervised"))
