"""bgs_canny_device without a GPU: the numpy restatement (tests/canny_numpy.py) against patterns worked out by hand, so that the
definition of DESIGN.md 5.12 is pinned independently of any kernel, and the entry point's refusals, which need no device.

The hand derivations use: a Sobel response of 4 * step across a straight step edge; magnitude 0 outside the image; `>` towards the
left / upper neighbour and `>=` towards the right / lower one for gradients along a row / column, `>` on both sides for diagonals."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import canny_numpy as cn
from tracking_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def img_of(rows):
    return np.array(rows, np.uint8)


def edges(rows):
    return (np.array([[c == "#" for c in r] for r in rows]) * 255).astype(np.uint8)


def test_tan_22_5_constant():
    assert cn.TG22 == 13573


def test_step_edge_5x5_keeps_the_left_of_two_equal_maxima():
    # columns 0, 1 dark, 2..4 bright: dx = 1020 in columns 1 and 2, 0 elsewhere, dy = 0.  Column 1 passes (1020 > 0 on its left,
    # 1020 >= 1020 on its right); column 2 fails (1020 > 1020 on its left).
    img = img_of([[0, 0, 255, 255, 255]] * 5)
    want = edges([".#..."] * 5)
    assert np.array_equal(cn.canny(img, 100, 150), want)
    # the same edge lying down: the upper of the two rows is kept
    assert np.array_equal(cn.canny(img.T, 100, 150), want.T)
    # a falling edge has the same magnitudes, so the same pixels
    assert np.array_equal(cn.canny(255 - img, 100, 150), want)


def test_sobel_of_the_step_edge():
    dx, dy = cn.sobel3(img_of([[0, 0, 255, 255, 255]] * 5))
    assert np.array_equal(dx, np.array([[0, 1020, 1020, 0, 0]] * 5)) and not dy.any()
    dx, dy = cn.sobel3(img_of([[0, 0, 255, 255, 255]] * 5).T)
    assert np.array_equal(dy, np.array([[0, 1020, 1020, 0, 0]] * 5).T) and not dx.any()


def test_one_pixel_vertical_and_horizontal_lines_7x7():
    # a bright column 3: dx = +1020 in column 2, -1020 in column 4, 0 in column 3; each flank is a maximum against 0 on both sides
    img = np.zeros((7, 7), np.uint8)
    img[:, 3] = 255
    want = edges(["..#.#.."] * 7)
    assert np.array_equal(cn.canny(img, 100, 150), want)
    assert np.array_equal(cn.canny(img.T, 100, 150), want.T)


@pytest.mark.parametrize("flip", [False, True])
def test_one_pixel_diagonal_lines_7x7(flip):
    # img[y][x] = 255 where x == y.  With k = x - y, away from the border: (dx, dy) / 255 = (1, -1), (2, -2), (0, 0), (-2, 2), (-1, 1)
    # for k = -2 .. 2, so the magnitudes are 510, 1020, 0, 1020, 510.  dx and dy have opposite signs: the pixels compared are
    # (y-1, x+1) and (y+1, x-1), that is k + 2 and k - 2.  k = -1 meets k = +1 with 1020 > 1020 false, and the other way round:
    # both are suppressed.  k = +-2 meet k = 0 and k = +-4, both 0: kept, and 510 is above 150.
    # Pixels less than 2 from the border see replicated rows and are left out of the hand check.
    img = (np.eye(7) * 255).astype(np.uint8)
    if flip:
        img = img[:, ::-1]  # the anti-diagonal: dx changes sign, the other diagonal class, the same magnitudes mirrored
    got = cn.canny(img, 100, 150)
    if flip:
        got = got[:, ::-1]
    want = edges(["..#",
                  "...",
                  "#.."])
    assert np.array_equal(got[2:5, 2:5], want)
    dx, dy = cn.sobel3((np.eye(7) * 255).astype(np.uint8))
    assert [int(dx[3, 3 + k]) // 255 for k in range(-2, 3)] == [1, 2, 0, -2, -1]
    assert [int(dy[3, 3 + k]) // 255 for k in range(-2, 3)] == [-1, -2, 0, 2, 1]


WEAK_AND_STRONG = img_of([[0, 0, 0, 255, 255, 255, 255]] * 3 + [[0, 0, 0, 35, 35, 35, 35]] * 4)


def test_weak_edge_attached_to_a_strong_one_7x7():
    # A step of 255 in rows 0..2 and of 35 in rows 3..6, between columns 2 and 3.
    # rows 0, 1: the plain step edge, magnitude 1020 in columns 2 and 3, column 2 kept: strong.
    # rows 4..6: the same with 4 * 35 = 140, between the thresholds: column 2 is a candidate only.
    # (2,2): dx = 255 + 510 + 35 = 800, dy = 35 - 255 = -220, along the row; its right neighbour (2,3) has dx = 800, dy = -660,
    #        magnitude 1460, so (2,2) is suppressed.  (2,3) is diagonal with signs opposed: against (1,4) = 0 and (3,2) = 580: strong.
    # (3,2): dx = 360, dy = -220, magnitude 580, diagonal, loses to (2,3).  (3,3): dx = 360, dy = -660, magnitude 1020, diagonal,
    #        against (2,4) = 880 and (4,2) = 140: strong, and it touches (4,2), which carries the edge down the weak part.
    # (2,4..6): dx = 0, dy = 4 * (35 - 255) = -880, along the column: 880 > 0 above and 880 >= 880 below: strong; row 3 loses (880 > 880).
    want = edges(["..#....",
                  "..#....",
                  "...####",
                  "...#...",
                  "..#....",
                  "..#....",
                  "..#...."])
    assert np.array_equal(cn.canny(WEAK_AND_STRONG, 100, 150), want)
    assert np.array_equal(cn.candidates(WEAK_AND_STRONG, 100, 150)[4:, 2], [1, 1, 1])
    assert np.array_equal(cn.canny(WEAK_AND_STRONG, 150, 100), want)  # the thresholds are ordered by the call
    # above the weak part's magnitude the lower half is gone; `>` is strict at exactly 140
    upper = want.copy()
    upper[4:] = 0
    assert np.array_equal(cn.canny(WEAK_AND_STRONG, 140, 150), upper)
    assert np.array_equal(cn.canny(WEAK_AND_STRONG, 139, 150), want)


def test_weak_edge_alone_7x7():
    img = img_of([[0, 0, 0, 35, 35, 35, 35]] * 7)  # magnitude 140 in columns 2 and 3
    assert np.array_equal(cn.candidates(img, 100, 150), (edges(["..#...."] * 7) // 255))
    assert not cn.canny(img, 100, 150).any()
    assert not cn.canny(img, 100, 140).any()  # 140 > 140 is false
    assert np.array_equal(cn.canny(img, 100, 139), edges(["..#...."] * 7))
    assert np.array_equal(cn.canny(img, 0, 0), edges(["..#...."] * 7))


def test_flat_images_have_no_edges():
    for v in (0, 255):
        assert not cn.canny(np.full((5, 7), v, np.uint8), 0, 0).any()


def test_checkerboard_has_no_gradient():
    # every 3x3 window of a one-pixel checkerboard has equal column sums and equal row sums away from the border; the replicated
    # border breaks that in the outer ring only
    yy, xx = np.mgrid[0:7, 0:7]
    img = (((yy + xx) & 1) * 255).astype(np.uint8)
    dx, dy = cn.sobel3(img)
    assert not dx[1:-1, 1:-1].any() and not dy[1:-1, 1:-1].any()
    assert not cn.canny(img, 0, 0)[1:-1, 1:-1].any()


# ---- the entry point ------------------------------------------------------------------------------------------------------------------

def test_header_declares_the_entry_point_and_its_limit():
    h = open(os.path.join(ROOT, "include", "bgs_hip.h")).read()
    assert re.search(r"int bgs_canny_device\(int hip_device, const void\* d_src, void\* d_dst, int images, int rows, int cols, int low, int high,\s*void\* hip_stream\);", h)
    m = re.search(r"#define BGS_CANNY_MAX_PIXELS (\d+)", h)
    assert m and int(m.group(1)) == capi.CANNY_MAX_PIXELS >= 160 * 120  # the reference's reduced frame fits


def test_refusals_need_no_device():
    f = capi.lib().bgs_canny_device
    a, b = C.c_void_p(0x1000), C.c_void_p(0x2000)  # never dereferenced: every call below is refused before any device work
    assert f(0, None, b, 1, 5, 5, 100, 150, None) == capi.ERR_INVALID
    assert f(0, a, None, 1, 5, 5, 100, 150, None) == capi.ERR_INVALID
    for images, rows, cols in ((0, 5, 5), (1, 0, 5), (1, 5, 0), (1, -1, 5), (65536, 5, 5)):
        assert f(0, a, b, images, rows, cols, 100, 150, None) == capi.ERR_INVALID, (images, rows, cols)
    assert f(0, a, a, 1, 5, 5, 100, 150, None) == capi.ERR_INVALID and "in-place" in capi.last_error()
    assert f(0, a, b, 1, 1, capi.CANNY_MAX_PIXELS + 1, 100, 150, None) == capi.ERR_UNSUPPORTED
    assert "bgs_canny_device" in capi.last_error() and "BGS_CANNY_MAX_PIXELS" in capi.last_error()
    assert f(0, a, b, 1, 46341, 46341, 100, 150, None) == capi.ERR_UNSUPPORTED  # rows * cols past 2^31 is not a small image
