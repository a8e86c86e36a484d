"""tests/flip_ref.py (the numpy restatement of flip-TTA that tests/test_flip_exact_gpu.py holds the engine to) against the
oracle, on the CPU:

* ``flip_tta_expected`` on the oracle's own plain and mirrored outputs is ``T.flip_tta_heatmaps`` bit for bit -- disjoint pairs,
  no pairs, pairs that share a joint;
* ``max_preds`` is ``T.max_preds_refined`` and the reference's stored decode (tests/golden), NaN / -inf / flat maps included;
* a crop that equals its own mirror image gives exact ties: every self-paired joint's averaged map is mirror-symmetric, its
  maximum is attained exactly twice and the first of the two lies in the left half; a swapped pair's maps mirror each other.
  The GPU tie cases rest on this."""
import numpy as np
import pytest
import torch

import flip_ref as F
from conftest import golden, load_pkg, state_dict_np
from oracle import hrnet_torch_oracle as T

NAME = "w32_128x96_fliptta_n3"
_PASSES = {}


def _sd(c=32, seed=0):
    return load_pkg().synth.to_torch_state_dict(state_dict_np(c, seed))


def _passes(h, w, n, seed):
    """crops, the oracle's plain pass and its pass on the mirrored crops (computed once, never modified)"""
    key = (h, w, n, seed)
    if key not in _PASSES:
        x = load_pkg().synth_crops(n, h, w, seed=seed)
        a = T.hrnet_forward(_sd(), torch.from_numpy(x)).numpy()
        b = T.hrnet_forward(_sd(), torch.flip(torch.from_numpy(x), dims=[-1])).numpy()
        for t in (a, b):
            t.setflags(write=False)
        _PASSES[key] = (x, a, b)
    return _PASSES[key]


@pytest.mark.parametrize("pairs", ["fixture", "none", "shared"])
def test_expected_is_the_oracles_flip_tta_bit_for_bit(pairs):
    pairs = {"fixture": golden(NAME)["flip_pairs"].tolist(), "none": [], "shared": F.SHARED_PAIRS}[pairs]
    x, a, b = _passes(64, 64, 2, 31)
    want = T.flip_tta_heatmaps(_sd(), torch.from_numpy(x), pairs).numpy()
    got = F.flip_tta_expected(a, b, pairs)
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got, want)
    if pairs:
        assert not np.array_equal(got, F.flip_tta_expected(a, b, []))        # the pairs matter on these maps


def test_shared_pairs_compose_in_order():
    """(1,2),(2,3) applied in place, one after the other: map 1 <- 2, map 2 <- 3, map 3 <- the old map 1"""
    b = np.arange(2 * 17 * 1 * 3, dtype=np.float32).reshape(2, 17, 1, 3)
    out = F.flip_back(b, F.SHARED_PAIRS)
    m = b[..., ::-1]
    src = {1: 2, 2: 3, 3: 1, 0: 16, 16: 0}
    for j in range(17):
        np.testing.assert_array_equal(out[:, j], m[:, src.get(j, j)])
    np.testing.assert_array_equal(b, np.arange(b.size, dtype=np.float32).reshape(b.shape))     # the argument is left alone


def test_max_preds_is_the_oracles_and_the_references_decode():
    g = golden(NAME)
    for pp, key in ((True, "preds"), (False, "preds_nopost")):
        preds, maxvals = F.max_preds(g["heatmaps"], pp)
        np.testing.assert_array_equal(preds, g[key])
        np.testing.assert_array_equal(maxvals, g["maxvals"])
        want = T.max_preds_refined(g["heatmaps"], pp)
        np.testing.assert_array_equal(preds, want[0])
        np.testing.assert_array_equal(maxvals, want[1])


def test_max_preds_on_non_finite_flat_and_tied_maps():
    rng = np.random.default_rng(5)
    hm = rng.standard_normal((1, 8, 8, 8)).astype(np.float32)
    hm[0, 0] = np.nan
    hm[0, 1] = -np.inf
    hm[0, 2] = 1.0
    hm[0, 3] = -1.0
    hm[0, 4] = 0.0
    hm[0, 5, 3, 4] = np.nan                          # one NaN in a finite map: it is the maximum
    hm[0, 6] = -np.abs(hm[0, 6]) - 1.0               # all negative: coordinates zeroed
    hm[0, 7, 2, 5] = hm[0, 7, 5, 2] = 9.0            # an exact tie: the first in row-major order
    for pp in (True, False):
        preds, maxvals = F.max_preds(hm, pp)
        want = T.max_preds_refined(hm, pp)
        np.testing.assert_array_equal(preds, want[0])
        np.testing.assert_array_equal(maxvals, want[1])
        assert np.isnan(maxvals[0, 0, 0]) and np.isneginf(maxvals[0, 1, 0]) and np.isnan(maxvals[0, 5, 0])
        np.testing.assert_array_equal(maxvals[0, [2, 3, 4, 7], 0], np.float32([1.0, -1.0, 0.0, 9.0]))
        np.testing.assert_array_equal(preds[0, :7], np.zeros((7, 2), np.float32))      # (joint 2: maximum at index 0)
        assert tuple(np.floor(preds[0, 7] + 0.5)) == (5.0, 2.0)


@pytest.mark.parametrize("h,w", [(32, 32), (64, 96)])
def test_symmetric_crops_give_exact_ties(h, w):
    xs = F.symmetric_crops(load_pkg().synth_crops(2, h, w, seed=37))
    np.testing.assert_array_equal(xs, xs[..., ::-1])
    pairs = [(1, 2), (3, 4)]
    own = [j for j in range(17) if j not in (1, 2, 3, 4)]
    a = T.hrnet_forward(_sd(), torch.from_numpy(xs)).numpy()
    b = T.hrnet_forward(_sd(), torch.flip(torch.from_numpy(xs), dims=[-1])).numpy()
    np.testing.assert_array_equal(a, b)                      # the same crops: the same pass
    hm = F.flip_tta_expected(a, b, pairs)
    np.testing.assert_array_equal(hm, T.flip_tta_heatmaps(_sd(), torch.from_numpy(xs), pairs).numpy())
    wq = w // 4
    np.testing.assert_array_equal(hm[:, own], hm[:, own][..., ::-1])
    for p0, p1 in pairs:
        np.testing.assert_array_equal(hm[:, p0], hm[:, p1][..., ::-1])
    flat = hm[:, own].reshape(2, len(own), -1)
    assert ((flat == flat.max(-1, keepdims=True)).sum(-1) == 2).all()       # the maximum and its mirror image, nothing else
    assert (flat.argmax(-1) % wq < wq // 2).all()                           # the first of the two: the left one
    for pp in (True, False):
        preds, maxvals = F.max_preds(hm, pp)
        want = T.max_preds_refined(hm, pp)
        np.testing.assert_array_equal(preds, want[0])
        np.testing.assert_array_equal(maxvals, want[1])
        seen = maxvals[:, own, 0] > 0
        assert seen.any() and (np.floor(preds[:, own, 0])[seen] < wq // 2).all()
