"""bgs_canny_device on the GPU against the numpy restatement (tests/canny_numpy.py, pinned by hand in tests/test_canny_cpu.py).
Every comparison is byte for byte."""
import numpy as np
import pytest

import canny_numpy as cn
from gpu_helpers import _torch
from tracking_amd import capi
from tracking_amd.engine import canny_device

pytestmark = pytest.mark.gpu

THRESHOLDS = [(100, 150), (0, 0)]


def on_device(img, low, high):
    torch = _torch()
    out = canny_device(torch.from_numpy(np.ascontiguousarray(img)).cuda(), low, high)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def checkerboard(rows, cols):
    yy, xx = np.mgrid[0:rows, 0:cols]
    return (((yy + xx) & 1) * 255).astype(np.uint8)


def blocks(rows, cols, seed):
    """8 x 8 blocks of random grey: long straight edges of every contrast, so hysteresis has chains to follow."""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, 256, ((rows + 7) // 8, (cols + 7) // 8), dtype=np.uint8)
    return np.ascontiguousarray(np.repeat(np.repeat(coarse, 8, 0), 8, 1)[:rows, :cols])


def snake(rows=120, cols=160):
    """A serpentine band 35 above a black ground with one bright patch at its start: with thresholds 100 / 250 only the patch is
    strong (a straight band edge has magnitude 140, a concave corner 210), and the edge has to be followed along the whole band."""
    img = np.zeros((rows, cols), np.uint8)
    j = 0
    while 8 * j + 6 <= rows - 2:
        img[8 * j + 2:8 * j + 6, 2:cols - 2] = 35
        if 8 * (j + 1) + 6 <= rows - 2:
            c = cols - 6 if j % 2 == 0 else 2
            img[8 * j + 6:8 * j + 10, c:c + 4] = 35
        j += 1
    img[2:6, 2:6] = 255
    return img


@pytest.mark.parametrize("low,high", THRESHOLDS)
@pytest.mark.parametrize("shape", [(7, 5), (64, 65), (33, 130)])
def test_noise(shape, low, high):
    img = np.random.default_rng(shape[0] * 1000 + shape[1]).integers(0, 256, shape, dtype=np.uint8)
    want = cn.canny(img, low, high)
    assert want.any() and not want.all()
    assert np.array_equal(on_device(img, low, high), want)


@pytest.mark.parametrize("low,high", THRESHOLDS)
@pytest.mark.parametrize("value", [0, 255])
def test_flat(value, low, high):
    got = on_device(np.full((33, 130), value, np.uint8), low, high)
    assert got.shape == (33, 130) and not got.any()


@pytest.mark.parametrize("low,high", THRESHOLDS)
def test_checkerboard(low, high):
    img = checkerboard(64, 65)
    want = cn.canny(img, low, high)
    assert not want[1:-1, 1:-1].any()
    assert np.array_equal(on_device(img, low, high), want)


@pytest.mark.parametrize("low,high", THRESHOLDS)
def test_batch_of_three(low, high):
    rng = np.random.default_rng(5)
    imgs = np.stack([rng.integers(0, 256, (33, 130), dtype=np.uint8), blocks(33, 130, 6), checkerboard(33, 130)])
    got = on_device(imgs, low, high)
    for k in range(3):
        assert np.array_equal(got[k], cn.canny(imgs[k], low, high)), k


def test_thresholds_are_ordered_by_the_call():
    img = blocks(64, 65, 7)
    assert np.array_equal(on_device(img, 150, 100), cn.canny(img, 100, 150))


@pytest.mark.parametrize("shape", [(1, 1), (1, 9), (9, 1), (2, 2)])
def test_degenerate_shapes(shape):
    img = np.random.default_rng(8).integers(0, 256, shape, dtype=np.uint8)
    assert np.array_equal(on_device(img, 0, 0), cn.canny(img, 0, 0))


def test_reduced_frame_size_blocks():
    img = blocks(120, 160, 9)
    want = cn.canny(img, 100, 150)
    cand = cn.candidates(img, 100, 150)
    assert (cand == 1).any() and ((cand == 1) & (want == 0)).any() and ((cand == 1) & (want == 255)).any()  # weak pixels kept and dropped
    assert np.array_equal(on_device(img, 100, 150), want)


def test_hysteresis_follows_a_long_chain():
    img = snake()
    want, cand = cn.canny(img, 100, 250), cn.candidates(img, 100, 250)
    assert (want == 255).sum() > 100 * (cand == 2).sum()  # nearly every edge pixel is reached from a few seeds
    assert np.array_equal(on_device(img, 100, 250), want)


def test_largest_image_and_the_refusal_above_it():
    torch = _torch()
    n = capi.CANNY_MAX_PIXELS
    img = blocks(n // 160, 160, 10)
    assert img.size == n
    assert np.array_equal(on_device(img, 100, 150), cn.canny(img, 100, 150))
    with pytest.raises(capi.BgsError) as e:
        canny_device(torch.zeros((n // 160 + 1, 160), dtype=torch.uint8, device="cuda"), 100, 150)
    assert e.value.code == capi.ERR_UNSUPPORTED and "BGS_CANNY_MAX_PIXELS" in str(e.value)
