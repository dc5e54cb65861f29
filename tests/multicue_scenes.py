"""Scripted frames, ghost maps and boxes for the model stage of SJN_MultiCueBGS (tests/multicue_numpy.py, tools/ref_fixtures/multicue).

scripted: a flat region (left 40 % of the columns), a static strong texture (the next 40 %) and per-frame uniform noise (the rest).
  After training a flat block appears, flickers between two colours, stands still long enough to be absorbed, moves away and
  leaves; the whole scene brightens by 40 at detecting frame 15.  Valid boxes follow the block and sit on the noise for a while,
  one box is invalid, and two frames carry a ghost rectangle.
drift: bred for codewords.  Stripes whose amplitude steps just past the texture range every frame beside a flat region whose grey
  level steps just past the colour range, both as triangle waves; a valid box covers the right half in alternate stretches."""
import numpy as np

NBOX = 3


def _interior_box(x0, x1, y0, y1, rw, rh, valid=1):
    """left, right, upper, bottom (inclusive) clamped to the interior, as the reference's boxes are"""
    return [max(2, min(x0, rw - 3)), max(2, min(x1, rw - 3)), max(2, min(y0, rh - 3)), max(2, min(y1, rh - 3)), valid]


def frames_of(gen, rows, cols, T, train, seed):
    rng = np.random.RandomState(seed)
    fr = np.zeros((T, rows, cols, 3), np.uint8)
    x = np.arange(cols)[None, :] / float(cols)
    y = np.arange(rows)[:, None] / float(rows)
    if gen == "drift":
        sgn = np.where(((np.arange(cols)[None, :] // 2 + np.arange(rows)[:, None] // 2) % 2) == 1, 1, -1)
        for t in range(T):
            amp = abs(((t * 9) % 220) - 110)
            grey = 20 + abs(((t * 23) % 420) - 210)
            img = np.where(x < 0.5, 128 + amp * sgn, grey)
            fr[t] = np.clip(img, 0, 255)[:, :, None]
        return fr
    assert gen == "scripted", gen
    texture = rng.randint(0, 256, (rows, cols, 1)) // 2 + 60
    base = np.where((x < 0.4)[:, :, None], np.array([90, 120, 150])[None, None, :], texture)
    noise_zone = np.broadcast_to(x >= 0.8, (rows, cols))
    A, B = np.array([200, 60, 60]), np.array([60, 200, 60])
    for t in range(T):
        img = base + rng.randint(-1, 2, (rows, cols, 3))
        d = t - train
        if d >= 15:
            img = img + 40
        if 2 <= d < 14:
            x0 = 0.25 + 0.1 * max(0, d - 8)
            blk = (x >= x0) & (x < x0 + 0.3) & (y >= 0.2) & (y < 0.6)
            img = np.where(blk[:, :, None], (B if d == 3 else A)[None, None, :], img)
        img = np.where(noise_zone[:, :, None], rng.randint(0, 256, (rows, cols, 3)), img)
        fr[t] = np.clip(img, 0, 255)
    return fr


def maps_of(gen, rh, rw, D):
    """(ghost [D][rh][rw] u8, boxes [D][NBOX][5] i16) in reduced coordinates"""
    ghost = np.zeros((D, rh, rw), np.uint8)
    boxes = np.zeros((D, NBOX, 5), np.int16)
    for d in range(D):
        if gen == "drift":
            if (d // 7) % 2 == 1:
                boxes[d, 0] = _interior_box(rw // 2, rw - 1, 0, rh - 1, rw, rh)
            continue
        if 2 <= d < 14:
            x0 = 0.25 + 0.1 * max(0, d - 8)
            boxes[d, 0] = _interior_box(int(x0 * rw) - 1, int((x0 + 0.3) * rw) + 1, int(0.2 * rh) - 1, int(0.6 * rh) + 1, rw, rh)
        if 3 <= d < 9:
            boxes[d, 1] = _interior_box(int(0.8 * rw), rw - 1, int(0.5 * rh), rh - 1, rw, rh)
        boxes[d, 2] = _interior_box(2, rw // 2, 2, rh // 2, rw, rh, valid=0)
        if d in (1, 10) and rw > 4 and rh > 4:
            ghost[d, 2:max(3, rh // 2), 2:max(3, rw // 3)] = 1
    return ghost, boxes


def update_map_of(boxes, rh, rw):
    """step 1 of UpdateModel_Par (:367-382): TRUE everywhere, FALSE inside the valid boxes"""
    m = np.ones((rh, rw), np.uint8)
    for l, r, u, b, v in boxes:
        if v:
            m[u:b + 1, l:r + 1] = 0
    return m
