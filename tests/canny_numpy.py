"""numpy restatement of bgs_canny_device: cvCanny with aperture 3 and the L1 magnitude.

Not a test module.  Written for clarity, not speed: whole-array numpy for the gradients, a plain worklist for the hysteresis.
"""
import numpy as np

TG22 = int(0.4142135623730950488016887242097 * (1 << 15) + 0.5)  # tan 22.5 deg in 15-bit fixed point = 13573


def sobel3(img):
    """3x3 Sobel derivatives of a uint8 image with a replicated border, as int32 (dx, dy)."""
    p = np.pad(img.astype(np.int32), 1, mode="edge")
    r, c = img.shape
    w = lambda dy, dx: p[1 + dy:1 + dy + r, 1 + dx:1 + dx + c]
    dx = (w(-1, 1) + 2 * w(0, 1) + w(1, 1)) - (w(-1, -1) + 2 * w(0, -1) + w(1, -1))
    dy = (w(1, -1) + 2 * w(1, 0) + w(1, 1)) - (w(-1, -1) + 2 * w(-1, 0) + w(-1, 1))
    return dx, dy


def candidates(img, low, high):
    """Non-maximum suppression.  Returns a uint8 map: 0 = no edge, 1 = above `low` and a local maximum, 2 = also above `high`."""
    if low > high:
        low, high = high, low
    dx, dy = sobel3(img)
    mag = np.abs(dx) + np.abs(dy)
    r, c = img.shape
    m = np.pad(mag, 1)  # the magnitude outside the image is 0
    at = lambda oy, ox: m[1 + oy:1 + oy + r, 1 + ox:1 + ox + c]
    x, y = np.abs(dx), np.abs(dy) << 15
    tg22x = x * TG22
    tg67x = tg22x + (x << 16)
    horiz = y < tg22x  # the gradient points along the row: compare left and right
    vert = ~horiz & (y > tg67x)
    diag = ~horiz & ~vert
    s_neg = (dx ^ dy) < 0  # dx and dy of opposite sign: the anti-diagonal
    keep_h = (mag > at(0, -1)) & (mag >= at(0, 1))
    keep_v = (mag > at(-1, 0)) & (mag >= at(1, 0))
    keep_d = np.where(s_neg, (mag > at(-1, 1)) & (mag > at(1, -1)), (mag > at(-1, -1)) & (mag > at(1, 1)))
    keep = (mag > low) & ((horiz & keep_h) | (vert & keep_v) | (diag & keep_d))
    return (keep.astype(np.uint8) + (keep & (mag > high)).astype(np.uint8))


def canny(img, low, high):
    """Edge map (0 / 255) of a uint8 [rows][cols] image."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    cand = candidates(img, low, high)
    r, c = cand.shape
    out = np.zeros((r, c), np.uint8)
    stack = [(int(y), int(x)) for y, x in zip(*np.nonzero(cand == 2))]
    for y, x in stack:
        out[y, x] = 255
    while stack:  # 8-connected growth from the strong pixels through the weak ones: a set, whatever the visiting order
        y, x = stack.pop()
        for ny in range(max(y - 1, 0), min(y + 2, r)):
            for nx in range(max(x - 1, 0), min(x + 2, c)):
                if cand[ny, nx] and not out[ny, nx]:
                    out[ny, nx] = 255
                    stack.append((ny, nx))
    return out
