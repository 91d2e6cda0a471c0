"""tests/thin_ref.py, the numpy restatement of hc_thinning_device, without a GPU: it agrees with the naive per-pixel restatement
iteration by iteration; subset, idempotence and (Guo-Hall) component-count properties on seeded blobs; the known answers of the
header's rules on blocks, rectangles and full frames; cut-and-continue."""
import numpy as np
import pytest

import thin_ref as T


@pytest.mark.parametrize("method", T.METHODS)
@pytest.mark.parametrize("density", [0.2, 0.5, 0.8])
def test_the_two_restatements_agree(method, density):
    rng = np.random.default_rng(int(density * 10) + 100 * method)
    for _ in range(3):
        m = rng.random((12, 20)) < density
        naive = [[int(v) for v in row] for row in m]
        for it in range(40):
            for s in (0, 1):   # the removals of either sub-iteration on the same map, pixel by pixel
                gone = T.removed_by(m, method, s)
                assert [tuple(int(v) for v in p) for p in np.argwhere(gone)] == T.removed_by_naive(naive, method, s), (it, s)
            m, r = T.iterate(m, method)
            naive, rn = T.iterate_naive(naive, method)
            assert r == rn and np.array_equal(m, np.array(naive, bool)), it
            if r == 0:
                break
        else:
            raise AssertionError("no fixed point in 40 iterations of a 12 x 20 frame")


def _components(m):
    from scipy import ndimage
    return ndimage.label(m != 0, structure=np.ones((3, 3), int))[1]


@pytest.mark.parametrize("method", T.METHODS)
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_properties_on_blobs(method, seed):
    m = T.blobs(48, 150, seed)
    assert 0.2 < (m != 0).mean() < 0.8
    out, it, conv = T.thin(m, method, 64)
    assert conv == 1 and it >= 2
    assert set(np.unique(out)) <= {0, 255}
    assert not (out & ~m).any(), "the output is a subset of the input"
    again, it2, conv2 = T.thin(out, method, 4)
    assert np.array_equal(again, out) and it2 == 0 and conv2 == 1, "thinning the output changes nothing"
    if method == T.GUOHALL:   # (Zhang-Suen erases 2 x 2 blocks: the known answers pin that)
        assert _components(out) == _components(m)


def _left(m, method, n=64):
    out, it, conv = T.thin(m, method, n)
    assert conv == 1
    return it, int((out != 0).sum())


def test_known_answers():
    block = np.zeros((6, 7), np.uint8)
    block[2:4, 3:5] = 1
    assert _left(block, T.ZHANGSUEN)[1] == 0 and _left(block, T.GUOHALL)[1] == 1
    rect = np.zeros((13, 40), np.uint8)
    rect[2:11, 3:37] = 255
    assert _left(rect, T.ZHANGSUEN) == (4, 25) and _left(rect, T.GUOHALL) == (4, 26)
    full = np.ones((9, 70), np.uint8)
    assert _left(full, T.ZHANGSUEN) == (4, 61) and _left(full, T.GUOHALL) == (4, 62)
    line = np.ones((1, 70), np.uint8)
    for method in T.METHODS:
        out, it, conv = T.thin(line, method, 16)
        assert (it, conv) == (0, 1) and (out == 255).all()


@pytest.mark.parametrize("method", T.METHODS)
def test_cut_and_continue(method):
    m = np.zeros((50, 60), np.uint8)
    m[4:44, 5:50] = 1
    full, total, conv = T.thin(m, method, 64)
    assert conv == 1 and total > 4
    for n1 in range(1, total):
        part, it1, c1 = T.thin(m, method, n1)
        assert (it1, c1) == (n1, 0)
        rest, it2, c2 = T.thin(part, method, 64)
        assert np.array_equal(rest, full) and it1 + it2 == total and c2 == 1
        exact, it3, c3 = T.thin(part, method, total - n1)   # exactly the remaining count: the fixed point, not yet known to be one
        assert np.array_equal(exact, full) and it3 == total - n1 and c3 == 0
    out, it, c = T.thin(m, method, total)
    assert np.array_equal(out, full) and (it, c) == (total, 0)
    out, it, c = T.thin(m, method, total + 1)
    assert np.array_equal(out, full) and (it, c) == (total, 1)


def test_max_iterations_range():
    for bad in (0, -1, 1025):
        with pytest.raises(ValueError):
            T.thin(np.ones((3, 3), np.uint8), T.ZHANGSUEN, bad)
