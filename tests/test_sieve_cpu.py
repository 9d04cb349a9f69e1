"""Minimum mapping unit, host half: hand-made cases of the oracle (tests/sieve_ref.py) that the GPU tests hold csrc/sieve.hip to, its
partition against scipy.ndimage.label where scipy is installed, the four entry points in the library and the binding, their argument
checks (which launch nothing) and the refusals of the Python wrappers.  No GPU."""
import ctypes

import numpy as np
import pytest

import sieve_ref
from kurosiwo_amd.scene import LABEL_TILE, component_sizes, label_components, sieve          # the feature under test: no GPU needed to import

ENTRIES = ("ksmi_scene_label", "ksmi_scene_component_sizes", "ksmi_scene_sieve_vote", "ksmi_scene_sieve_apply")


def _map(rows):
    return np.asarray(rows, dtype=np.uint8)


def test_a_diagonal_pair_is_two_components_at_4_and_one_at_8():
    m = _map([[1, 0], [0, 1]])
    assert sieve_ref.label(m, 4).tolist() == [[0, 1], [2, 3]]
    assert sieve_ref.label(m, 8).tolist() == [[0, 1], [1, 0]]
    assert sieve_ref.sizes(sieve_ref.label(m, 8)).tolist() == [[2, 2], [0, 0]]
    with pytest.raises(ValueError):
        sieve_ref.label(m, 5)


def test_labels_are_minimum_linear_indices_and_sizes_sit_at_roots():
    m = _map([[0, 0, 1, 1, 0],
              [1, 0, 1, 0, 0],
              [1, 1, 1, 0, 2]])
    lab = sieve_ref.label(m, 4)
    assert lab.dtype == np.int32
    assert lab.tolist() == [[0, 0, 2, 2, 4], [2, 0, 2, 4, 4], [2, 2, 2, 4, 14]]
    size = sieve_ref.sizes(lab)
    assert size.dtype == np.int32 and size.sum() == m.size
    assert size.ravel()[[0, 2, 4, 14]].tolist() == [3, 7, 4, 1] and np.count_nonzero(size) == 4


def test_a_component_of_exactly_mmu_pixels_is_kept_and_one_pixel_fewer_is_removed():
    m = np.zeros((7, 9), np.uint8)
    m[1, 1:5] = 1                         # 4 pixels
    m[4, 2:5] = 1                         # 3 pixels
    out, removed = sieve_ref.sieve(m, 4)
    want = m.copy()
    want[4, 2:5] = 0
    assert np.array_equal(out, want) and removed == 1
    assert sieve_ref.census(m, 4) == (1, 2, 1, 1)
    out, removed = sieve_ref.sieve(m, 5)
    assert not out.any() and removed == 2


def test_a_tie_goes_to_the_lowest_class():
    for left, right in ((0, 1), (1, 0)):
        m = np.full((5, 6), right, np.uint8)
        m[:, :3] = left
        m[2, 2:4] = 2                     # two pixels astride the seam: 3 votes from each side
        out, removed = sieve_ref.sieve(m, 3)
        assert out[2, 2] == 0 and out[2, 3] == 0 and removed == 1
        m[2, 1] = 2                       # three pixels: 5 votes from the left class, 3 from the right
        out, _ = sieve_ref.sieve(m, 4)
        assert (out[2, 1:4] == left).all()


def test_an_island_inside_invalid_pixels_is_kept():
    m = np.zeros((7, 7), np.uint8)
    m[2:5, 2:5] = 3
    m[3, 3] = 1                           # bounded by invalid pixels only
    m[0, 0] = 2                           # bounded by the scene border and the background
    out, removed = sieve_ref.sieve(m, 4)
    want = m.copy()
    want[0, 0] = 0
    assert np.array_equal(out, want) and removed == 1


def test_two_adjacent_specks_do_not_swap_and_a_checkerboard_does_not_invert():
    m = np.zeros((5, 6), np.uint8)
    m[2, 2], m[2, 3] = 1, 2
    out, removed = sieve_ref.sieve(m, 2)
    assert not out.any() and removed == 2
    board = (np.add.outer(np.arange(6), np.arange(7)) & 1).astype(np.uint8)
    out, removed = sieve_ref.sieve(board, 2, connectivity=4)
    assert np.array_equal(out, board) and removed == 0             # every pixel is small: nobody may vote


def test_an_invalid_blob_is_never_changed_and_never_donates():
    m = np.zeros((6, 8), np.uint8)
    m[0:3, 0:4] = 3                       # a large invalid blob
    m[5, 6:8] = 3                         # a small one
    m[3, 1] = 1                           # a speck under the blob: invalid above, background on three sides
    m[1, 4] = 2                           # a speck beside it: invalid to the left
    out, removed = sieve_ref.sieve(m, 3)
    want = m.copy()
    want[3, 1] = want[1, 4] = 0
    assert np.array_equal(out, want) and removed == 2
    # a speck whose only large neighbours are invalid keeps its class
    n = np.full((5, 5), 3, np.uint8)
    n[2, 2] = 1
    out, removed = sieve_ref.sieve(n, 3)
    assert np.array_equal(out, n) and removed == 0
    # another invalid class: value 7 with three classes; a value without a row in the vote table counts as invalid too
    k = np.zeros((5, 5), np.uint8)
    k[2, 2], k[0, 0] = 7, 5
    out, removed = sieve_ref.sieve(k, 3, invalid_class=7, num_classes=3)
    assert np.array_equal(out, k) and removed == 0


def test_mmu_of_one_or_less_is_the_identity():
    m = sieve_ref.speckle_scene(7, 20, 30)
    for mmu in (1, 0, -3):
        for conn in (4, 8):
            out, removed = sieve_ref.sieve(m, mmu, conn)
            assert np.array_equal(out, m) and removed == 0


def test_a_second_pass_dissolves_a_cluster_that_one_pass_keeps():
    m = np.zeros((7, 7), np.uint8)
    m[3, 3] = 1
    m[2, 3] = m[4, 3] = m[3, 2] = m[3, 4] = 2                       # four specks around a speck: its neighbours are all small
    one, removed = sieve_ref.sieve(m, 2)
    want = np.zeros((7, 7), np.uint8)
    want[3, 3] = 1
    assert np.array_equal(one, want) and removed == 4
    two, removed = sieve_ref.sieve(m, 2, passes=2)
    assert not two.any() and removed == 5


def test_the_speckle_scene_is_what_its_docstring_says():
    m = sieve_ref.speckle_scene(5, 65, 129)
    assert m.dtype == np.uint8 and m.shape == (65, 129) and np.array_equal(m, sieve_ref.speckle_scene(5, 65, 129))
    share = np.bincount(m.ravel(), minlength=4) / m.size
    assert abs(share[3] - 0.01) < 0.005 and 0.5 < share[0] < 0.65 and 0.2 < share[1] < 0.3 and 0.1 < share[2] < 0.2


@pytest.mark.parametrize("conn", (4, 8))
def test_the_oracle_partitions_as_scipy_does(conn):
    ndimage = pytest.importorskip("scipy.ndimage")
    structure = np.ones((3, 3), int) if conn == 8 else None
    for seed, shape in ((5, (65, 129)), (2, (96, 96)), (3, (130, 67))):
        m = sieve_ref.speckle_scene(seed, *shape)
        box = ndimage.uniform_filter(np.random.default_rng(seed).standard_normal(shape), 9, mode="nearest")
        assert np.abs(box - sieve_ref.box_mean9(np.random.default_rng(seed).standard_normal(shape))).max() < 1e-12
        lab = sieve_ref.label(m, conn)
        for c in range(4):
            theirs, n = ndimage.label(m == c, structure)
            mask = m == c
            pairs = np.unique(np.stack((lab[mask], theirs[mask])), axis=1)
            assert pairs.shape[1] == n == len(np.unique(lab[mask]))          # one of ours per one of theirs, both ways
        ys, xs = np.divmod(lab, m.shape[1])
        assert np.array_equal(m[ys, xs], m)                                  # a root has its component's class
        assert (lab.ravel() <= np.arange(m.size)).all()


def test_library_exports_and_binds_the_sieve_entry_points():
    from kurosiwo_amd import _lib
    lib = _lib.load()
    for name in ENTRIES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and args[-1] is ctypes.c_void_p          # int status, the stream last
    assert lib.ksmi_abi_version() == 8


def test_argument_errors_launch_nothing_and_name_the_entry_point():
    from kurosiwo_amd import _lib
    lib = _lib.load()
    P = 0x1000                                                              # never dereferenced: every case fails before a launch
    big = 1 << 31

    def refused(entry, rc):
        assert rc < 0
        assert entry in lib.ksmi_last_error().decode()

    label = lambda c=P, Hs=16, Ws=16, conn=4, out=P: lib.ksmi_scene_label(c, Hs, Ws, conn, out, None)
    for kw in (dict(c=None), dict(out=None), dict(conn=5), dict(conn=0), dict(Hs=0), dict(Ws=0), dict(Hs=-1), dict(Hs=65536, Ws=32768)):
        refused("scene_label", label(**kw))
    size = lambda lab=P, HW=256, out=P: lib.ksmi_scene_component_sizes(lab, HW, out, None)
    for kw in (dict(lab=None), dict(out=None), dict(HW=-1), dict(HW=big)):
        refused("scene_component_sizes", size(**kw))
    assert size(HW=0) == 0 and size(lab=None, HW=0) == 0
    vote = lambda c=P, lab=P, sz=P, inv=3, K=4, Hs=16, Ws=16, v=P: lib.ksmi_scene_sieve_vote(c, lab, sz, 4, inv, K, Hs, Ws, v, None)
    for kw in (dict(c=None), dict(lab=None), dict(sz=None), dict(v=None), dict(K=0), dict(K=9), dict(Hs=0), dict(Ws=-2), dict(inv=256),
               dict(inv=-1), dict(Hs=65536, Ws=32768)):
        refused("scene_sieve_vote", vote(**kw))
    apply = lambda c=P, lab=P, sz=P, v=P, inv=3, K=4, HW=256, out=P, rem=P: lib.ksmi_scene_sieve_apply(c, lab, sz, v, 4, inv, K, HW, out, rem, None)
    for kw in (dict(c=None), dict(lab=None), dict(sz=None), dict(v=None), dict(out=None), dict(rem=None), dict(K=0), dict(K=9), dict(HW=-1),
               dict(HW=big), dict(inv=300)):
        refused("scene_sieve_apply", apply(**kw))
    assert apply(HW=0) == 0
    th, tw = LABEL_TILE
    assert th >= 1 and tw >= 1 and th * tw <= 4096


def test_the_wrappers_refuse_cpu_tensors_and_bad_arguments():
    import torch
    from kurosiwo_amd import _lib
    from kurosiwo_amd.scene import predict_scene
    m = torch.zeros((8, 8), dtype=torch.uint8)
    with pytest.raises(_lib.KsmiError):
        label_components(m)
    with pytest.raises(_lib.KsmiError):
        component_sizes(torch.zeros((8, 8), dtype=torch.int32))
    with pytest.raises(_lib.KsmiError):
        sieve(m, 4)
    for bad in (lambda: label_components(m, connectivity=5), lambda: sieve(m, 4, connectivity=6), lambda: sieve(m, 4, num_classes=0),
                lambda: sieve(m, 4, num_classes=9), lambda: sieve(m, 4, passes=0), lambda: sieve(m, 4, invalid_class=256),
                lambda: predict_scene(None, [m], [None], mmu=4, connectivity=5)):
        with pytest.raises(ValueError):
            bad()
