"""numpy restatement of the box stage of SJN_MultiCueBGS (package_bgs/sjn/SJN_MultiCueBGS.cpp:335, :367-382) and of the
whole-frame step (process(), :85-99) on top of tests/multicue_numpy.py, which it imports unchanged.

Not a test module.  Written for clarity: the labelling is the reference's two raster loops as they stand, the Canny is
tests/canny_numpy.py.  Pinned byte for byte to the reference's own code by tests/golden/multicue_box_ref.npz (tools/ref_fixtures/multicue).
"""
import numpy as np

import canny_numpy
import multicue_numpy as mc

MAX_BOXES = 300  # BGS_MULTICUE_MAX_BOXES, the reference's iElementNum (:175)
BOX_FIELDS = ("rleft", "rright", "rupper", "rbottom", "left", "right", "upper", "bottom", "size_valid", "valid", "frame_edges", "fore_edges", "near")
CANNY_LOW, CANNY_HIGH = 100, 150
GHOST_DIST2 = 100  # dThreshold 10, squared


def majority(landmark):
    """MorphologicalOpearions(..., 0.5, 5, ...) (:671): 255 where at least (int)(25 * 0.5) pixels of the 5 x 5 window EQUAL 255"""
    rh, rw = landmark.shape
    out = np.zeros((rh, rw), np.uint8)
    if rh < 5 or rw < 5:
        return out
    e = (landmark == 255).astype(np.int32)
    c = sum(e[2 + dy:rh - 2 + dy, 2 + dx:rw - 2 + dx] for dy in range(-2, 3) for dx in range(-2, 3))
    out[2:rh - 2, 2:rw - 2] = np.where(c >= int(25 * 0.5), 255, 0)
    return out


def labeling(fore):
    """Labeling (:720) as written.  Returns (label table int32 [rh][rw], label count, stats)."""
    rh, rw = fore.shape
    p1 = [[0] * rw for _ in range(rh)]
    t1 = list(range(rh * rw // 2 + 1))
    f = (fore == 255).tolist()
    cnt = merges = up_plus_le = 0
    for y in range(1, rh):
        row, above, fy = p1[y], p1[y - 1], f[y]
        for x in range(1, rw):
            if not fy[x]:
                continue
            up, le = above[x], row[x - 1]
            if up == 0 and le == 0:
                cnt += 1
                row[x] = cnt
            elif up != 0 and le != 0:
                if up > le:
                    row[x] = le
                    t1[up] = t1[le]
                else:
                    row[x] = up
                    t1[le] = t1[up]
                merges += up != le
            else:
                row[x] = up + le
                up_plus_le += 1
    t2, label = {}, 0
    lab = np.zeros((rh, rw), np.int32)
    for y in range(1, rh):
        for x in range(1, rw):
            if p1[y][x]:
                v = t1[p1[y][x]]
                if v not in t2:
                    label += 1
                    t2[v] = label
                lab[y, x] = t2[v]
    return lab, label, {"pass1_labels": cnt, "merges": merges, "up_plus_le": up_plus_le}


def blobs4(fore):
    """4-connected components of fore == 255 (what a resolved labelling would give): int32 table, count.  For the fixture's branch counts."""
    rh, rw = fore.shape
    out = np.zeros((rh, rw), np.int32)
    n = 0
    for y0, x0 in zip(*np.nonzero(fore == 255)):
        if out[y0, x0]:
            continue
        n += 1
        out[y0, x0] = n
        stack = [(int(y0), int(x0))]
        while stack:
            y, x = stack.pop()
            for yy, xx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
                if 0 <= yy < rh and 0 <= xx < rw and fore[yy, xx] == 255 and not out[yy, xx]:
                    out[yy, xx] = n
                    stack.append((yy, xx))
    return out, n


def _short(v):
    return ((int(v) + 32768) % 65536) - 32768


def bounding_boxes(lab, count, H, W):
    """SetBoundingBox (:807) and EvaluateBoxSize (:886): int32 [count][13], the ghost columns still 0"""
    rh, rw = lab.shape
    b = np.zeros((count, len(BOX_FIELDS)), np.int32)
    bw, bh = rw // 80, rh // 60
    lo_w, lo_h = max(rw // 32, 5), max(rh // 24, 5)
    hr, wr = np.float64(H) / np.float64(rh), np.float64(W) / np.float64(rw)
    for k in range(count):
        ys, xs = np.nonzero(lab == k + 1)
        le, ri, up, bo = int(xs.min()) - bw, int(xs.max()) + bw, int(ys.min()) - bh, int(ys.max()) + bh
        le, up = max(le, 2), max(up, 2)
        if ri >= rw - 2:
            ri = rw - 3
        if bo >= rh - 2:
            bo = rh - 3
        b[k, 0:4] = le, ri, up, bo
        b[k, 4:8] = _short(int(le * wr)), _short(int(ri * wr)), _short(int(up * hr)), _short(int(bo * hr))
        w, h = ri - le, bo - up
        b[k, 8] = b[k, 9] = lo_w <= w <= rw and lo_h <= h <= rh
    return b


def resize_nn(frame, rh, rw):
    """cvResize(CV_INTER_NN) as OpenCV 2.4's resizeNN is recalled (unpinned): min(floor(i * (1.0 / ((double)rh / H))), H - 1)"""
    H, W = frame.shape[:2]
    sy = np.minimum(np.floor(np.arange(rh, dtype=np.float64) * (1.0 / (np.float64(rh) / np.float64(H)))).astype(np.int64), H - 1)
    sx = np.minimum(np.floor(np.arange(rw, dtype=np.float64) * (1.0 / (np.float64(rw) / np.float64(W)))).astype(np.int64), W - 1)
    return frame[sy][:, sx], sy, sx


def grey(bgr):
    """cvCvtColor(CV_BGR2GRAY) on bytes (recalled, unpinned)"""
    v = bgr.astype(np.int64)
    return ((v[..., 0] * 1868 + v[..., 1] * 9617 + v[..., 2] * 4899 + 8192) >> 14).astype(np.uint8)


def _sat_short(v):
    return np.clip(np.rint(v), -32768, 32767).astype(np.int64)


def _linear_axis(d, s):
    scale = 1.0 / (np.float64(d) / np.float64(s))
    f = ((np.arange(d, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    i = np.floor(f).astype(np.int64)
    f = f - i.astype(np.float32)
    return f, i


def resize_linear(src, drows, dcols):
    """cvResize (bilinear) of one 8-bit channel as oracle/ingest_oracle.c states it (recalled, unpinned): 11-bit coefficients, and the
    2 x 2 mean for an exact 2x reduction"""
    srows, scols = src.shape
    s = src.astype(np.int64)
    if srows == 2 * drows and scols == 2 * dcols:
        return ((s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    fx, sx = _linear_axis(dcols, scols)
    fx = np.where((sx < 0) | (sx >= scols - 1), np.float32(0), fx)
    sx = np.clip(sx, 0, scols - 1)
    sx1 = np.minimum(sx + 1, scols - 1)
    a0, a1 = _sat_short((np.float32(1) - fx) * np.float32(2048)), _sat_short(fx * np.float32(2048))
    fy, sy = _linear_axis(drows, srows)
    b0, b1 = _sat_short((np.float32(1) - fy) * np.float32(2048)), _sat_short(fy * np.float32(2048))
    S0, S1 = s[np.clip(sy, 0, srows - 1)], s[np.clip(sy + 1, 0, srows - 1)]
    r0 = S0[:, sx] * a0[None, :] + S0[:, sx1] * a1[None, :]
    r1 = S1[:, sx] * a0[None, :] + S1[:, sx1] * a1[None, :]
    out = (((b0[:, None] * (r0 >> 4)) >> 16) + ((b1[:, None] * (r1 >> 4)) >> 16) + 2) >> 2
    return (out & 0xff).astype(np.uint8)


def edge_counts(edge_frame, edge_fore):
    """(frame-edge points, foreground-edge points, foreground-edge points with a frame-edge point within squared distance 100)"""
    ay, ax = np.nonzero(edge_frame)
    by, bx = np.nonzero(edge_fore)
    if not len(ay) or not len(by):
        return len(ay), len(by), 0
    d2 = (by[:, None] - ay[None, :]) ** 2 + (bx[:, None] - ax[None, :]) ** 2
    return len(ay), len(by), int((d2.min(1) <= GHOST_DIST2).sum())


def ghost_by_count(na, nb, near):
    """distance > 10 of CalculateHausdorffDist (:1056), decided without a sort or a square root: the squared distances are integers, so
    sqrt(d[(int)(0.9 n)]) > 10 <=> d[(int)(0.9 n)] > 100 <=> at most (int)(0.9 n) of them are <= 100"""
    if na == 0 or nb == 0:
        return max(na, nb) > 10  # the size of the other set; both empty: 0
    return near <= int(0.9 * nb)


def hausdorff(edge_frame, edge_fore):
    """CalculateHausdorffDist as written, the double it returns"""
    ay, ax = np.nonzero(edge_frame)
    by, bx = np.nonzero(edge_fore)
    if not len(ay) or not len(by):
        return float(max(len(ay), len(by)))
    d2 = ((by[:, None] - ay[None, :]) ** 2 + (bx[:, None] - ax[None, :]) ** 2).min(1).astype(np.float64)
    d2.sort()
    i = int(0.9 * len(d2))
    if i == len(d2):
        i -= 1
    return float(np.sqrt(d2[i]))


def boxes(landmark, frame, windows=None):
    """PostProcessing (:335) and step 1 of UpdateModel_Par (:367-382) on one landmark map [rh][rw] and one frame [H][W][3].
    Returns a dict: fore, ghost, update u8 [rh][rw]; count; boxes int32 [min(count, 300)][13]; fore0 (before any removal); stats.
    `windows`, a list, receives (grey window, frame edges, foreground window, foreground edges) of every box that passed the size test."""
    rh, rw = landmark.shape
    H, W = frame.shape[:2]
    fore0 = majority(landmark)
    lab, count, stats = labeling(fore0)
    kept = min(count, MAX_BOXES)
    b = bounding_boxes(lab, kept, H, W)
    g = grey(resize_nn(frame, rh, rw)[0])
    fore, ghost, update = fore0.copy(), np.zeros((rh, rw), np.uint8), np.ones((rh, rw), np.uint8)
    for k in range(kept):
        le, ri, up, bo = (int(v) for v in b[k, 0:4])
        if not b[k, 8]:
            continue
        gw, fw = np.ascontiguousarray(g[up:bo, le:ri]), np.ascontiguousarray(fore0[up:bo, le:ri])
        ea, eb = canny_numpy.canny(gw, CANNY_LOW, CANNY_HIGH), canny_numpy.canny(fw, CANNY_LOW, CANNY_HIGH)
        if windows is not None:
            windows.append((gw, ea, fw, eb))
        na, nb, near = edge_counts(ea, eb)
        b[k, 10:13] = na, nb, near
        if ghost_by_count(na, nb, near):
            ghost[up:bo, le:ri] = 1
            b[k, 9] = 0
    for k in range(kept):
        le, ri, up, bo = (int(v) for v in b[k, 0:4])
        if b[k, 9]:
            update[up:bo + 1, le:ri + 1] = 0
        else:
            fore[up:bo, le:ri] = 0  # only 255s are there to be zeroed
    return {"fore": fore, "ghost": ghost, "update": update, "count": count, "boxes": b, "fore0": fore0, "labels": lab, "stats": stats,
            "box_overflow": int(count > MAX_BOXES)}


def box_rows(b):
    """[MAX_BOXES][13] with the rows at and beyond the count 0, as bgs_multicue_boxes_device writes them"""
    out = np.zeros((MAX_BOXES, len(BOX_FIELDS)), np.int32)
    out[:len(b)] = b
    return out


class Step:
    """process() (:85-99) on one stream: training frames give zeros, afterwards the landmark map, the box stage, the ghost update, the
    update and GetForegroundMap(result, NULL) = the foreground map resized bilinearly to the frame"""

    def __init__(self, params=None):
        self.m = mc.Model(params)
        self.box_overflow = 0
        self.last = None

    def process(self, frame):
        frame = np.asarray(frame)
        H, W = frame.shape[:2]
        if self.m.count <= self.m.p["training_period"]:
            self.m.train(frame)
            return np.zeros((H, W), np.uint8)
        lm, _ = self.m.landmark_map(frame)
        r = boxes(lm, frame)
        self.box_overflow += r["box_overflow"]
        self.m.update(r["ghost"], True)
        self.m.update(r["update"], False)
        self.last = r
        return resize_linear(r["fore"], H, W)


# ---- seeded blob masks: rectangles and discs, not dense noise

def blob_landmark(rh, rw, seed, blobs=6):
    """A landmark map (0 / 125 / 255) of `blobs` rectangles and discs and a little 125"""
    rng = np.random.RandomState(seed)
    lm = np.zeros((rh, rw), np.uint8)
    yy, xx = np.mgrid[0:rh, 0:rw]
    for i in range(blobs):
        cy, cx = rng.randint(0, rh), rng.randint(0, rw)
        ry, rx = rng.randint(2, max(3, rh // 4)), rng.randint(2, max(3, rw // 4))
        if i % 2:
            lm[((yy - cy) * rx) ** 2 + ((xx - cx) * ry) ** 2 <= (ry * rx) ** 2] = 255
        else:
            lm[max(cy - ry, 0):cy + ry, max(cx - rx, 0):cx + rx] = 255
    lm[rng.rand(rh, rw) < 0.03] = 125
    lm[[0, 1, rh - 2, rh - 1], :] = 0
    lm[:, [0, 1, rw - 2, rw - 1]] = 0
    return lm


def blob_frame(rows, cols, landmark, seed, follow=0.5):
    """A frame whose objects follow about `follow` of the landmark's columns (valid boxes there, ghosts elsewhere), on a dark ramp"""
    rng = np.random.RandomState(seed + 1000)
    rh, rw = landmark.shape
    sy = (np.arange(rows) * rh) // rows
    sx = (np.arange(cols) * rw) // cols
    big = landmark[sy][:, sx] == 255
    keep = np.broadcast_to((np.arange(cols)[None, :] < cols * follow), big.shape)
    img = np.full((rows, cols, 3), 40, np.int64) + (np.arange(cols)[None, :, None] % 7)
    img[big & keep] = (200, 180, 220)
    if rows >= 8 and cols >= 8:  # a stripe pattern with edges of its own on the far side
        img[:, cols - cols // 6:] += ((np.arange(rows)[:, None, None] // 3) % 2) * 120
    img += rng.randint(0, 3, img.shape)
    return np.clip(img, 0, 255).astype(np.uint8)


def hand_case(rh, rw, rows, cols, seed):
    """(landmark [rh][rw], frame [rows][cols][3]) drawn on a 30 x 40 grid and scaled up by rh // 30: a spiral whose bridge gets a label
    that is copied before the label it was copied from is merged (one blob, two labels); a thin tall bar and a flat wide bar for the
    size test; an L whose rectangle holds part of a separate dot; a patch of 125.  The frame shows the objects of the left half only
    (the L is a ghost with no frame edges) and only the left end of the flat bar (a ghost by distance where the bar is large enough)."""
    s = rh // 30
    assert s >= 1 and rh == 30 * s and rw == 40 * s
    lm, obj = np.zeros((30, 40), np.uint8), np.zeros((30, 40), bool)

    def rect(r0, r1, c0, c1, show=None):
        lm[r0:r1 + 1, c0:c1 + 1] = 255
        if show is None:
            show = c1 < 20
        if show:
            obj[r0:r1 + 1, c0:c1 + 1] = True

    rect(3, 20, 3, 8), rect(15, 20, 3, 16)                      # the spiral's trunk and lower bar
    rect(3, 9, 22, 27, False), rect(10, 14, 13, 27, False)      # its block on the right and the bridge coming back
    obj[10:15, 13:20] = True
    rect(3, 10, 32, 35)                                         # thin and tall
    rect(23, 26, 3, 20, False)                                  # flat and wide
    obj[23:27, 3:9] = True
    rect(19, 27, 23, 27), rect(23, 27, 23, 37), rect(15, 19, 32, 36)  # the L and the dot
    lm[28:30, 10:14] = 125
    lm = np.kron(lm, np.ones((s, s), np.uint8))
    obj = np.kron(obj.astype(np.uint8), np.ones((s, s), np.uint8)).astype(bool)
    rng = np.random.RandomState(seed)
    big = obj[(np.arange(rows) * rh) // rows][:, (np.arange(cols) * rw) // cols]
    img = np.full((rows, cols, 3), 50, np.int64)
    img[big] = (210, 190, 230)
    img += rng.randint(0, 3, img.shape)
    return lm, np.clip(img, 0, 255).astype(np.uint8)


def grid_landmark(rh, rw, blocks):
    """`blocks` blocks of 4 x 3 pixels of 255 (12, the filter's threshold) on a pitch of 6: the majority filter leaves 2 x 3 pixels of
    each, no window reaches 12 across two blocks, so every block is one label"""
    lm = np.zeros((rh, rw), np.uint8)
    per_row = (rw - 4) // 6
    assert blocks <= per_row * ((rh - 4) // 6), "the grid does not fit"
    for k in range(blocks):
        y, x = 2 + 6 * (k // per_row), 2 + 6 * (k % per_row)
        lm[y:y + 4, x:x + 3] = 255
    return lm


def post_inputs():
    """The hand-made inputs of the fixture's box-stage cases: (name, rh, rw, frame rows, cols, landmark, frame)"""
    out = []
    for name, rh, rw, rows, cols, seed in (("blobs_12x16", 12, 16, 24, 32, 31), ("blobs_30x40", 30, 40, 45, 70, 32), ("blobs_17x70", 17, 70, 40, 150, 33),
                                           ("blobs_120x160_39x52", 120, 160, 39, 52, 34), ("blobs_120x160_80x96", 120, 160, 80, 96, 35)):
        lm = blob_landmark(rh, rw, seed)
        out.append((name, rh, rw, rows, cols, lm, blob_frame(rows, cols, lm, seed)))
    full = np.full((120, 160), 255, np.uint8)  # one box with the largest window there is: columns 2..157, rows 2..117
    out.append(("largest_window", 120, 160, 240, 320, full, blob_frame(240, 320, majority(full), 36, follow=1.0)))
    out.append(("largest_window_ghost", 120, 160, 240, 320, full, blob_frame(240, 320, np.zeros((120, 160), np.uint8), 37)))
    small = np.full((12, 16), 255, np.uint8)  # the smallest size with a box that passes the 5-pixel test; a flat frame: no edge on either side
    out.append(("full_12x16_flat", 12, 16, 24, 32, small, np.full((24, 32, 3), 60, np.uint8)))
    grid = grid_landmark(120, 160, MAX_BOXES)
    out.append(("grid_300", 120, 160, 120, 160, grid, blob_frame(120, 160, grid, 38)))
    for name, rh, rw, rows, cols, seed in (("hand_30x40", 30, 40, 60, 80, 41), ("hand_60x80", 60, 80, 60, 80, 42)):
        lm, fr = hand_case(rh, rw, rows, cols, seed)
        out.append((name, rh, rw, rows, cols, lm, fr))
    return out


_FIXTURE = None


def load():
    """tests/golden/multicue_box_ref.npz as {"post": {case: record}, "step": {case: record}, "branches": {...}}.  The inputs are made
    again (post_inputs, tests/multicue_scenes.py) and checked against the stored CRCs; maps are unpacked to u8 0 / 1."""
    global _FIXTURE
    if _FIXTURE is None:
        import os
        import multicue_scenes as sc
        z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "multicue_box_ref.npz"))
        out = {"post": {}, "step": {}, "branches": dict(zip((str(k) for k in z["branch_names"]), (int(v) for v in z["branches"])))}

        def maps(name, shape):
            n = int(np.prod(shape))
            return {k: np.unpackbits(z[name + "." + k])[:n].reshape(shape) for k in ("fore", "ghost", "update")}

        inputs = {c[0]: c for c in post_inputs()}
        for name in (str(c) for c in z["post_cases"]):
            _, rh, rw, rows, cols, lm, frame = inputs[name]
            assert [rh, rw, rows, cols] == [int(v) for v in z[name + ".geom"]], name
            assert [mc.crc(lm), mc.crc(frame)] == [int(v) for v in z[name + ".input_crc"]], name
            r = dict(maps(name, (rh, rw)), landmark=lm, frame=frame, boxes=z[name + ".boxes"].astype(np.int32), dist=z[name + ".dist"])
            r["count"] = len(r["boxes"])
            out["post"][name] = r
        for name in (str(c) for c in z["step_cases"]):
            p = {k: (int(v) if k in mc.INT_FIELDS else float(v)) for k, v in zip(mc.FIELDS, z[name + ".params"])}
            rows, cols, T, seed = (int(v) for v in z[name + ".geom"])
            train = p["training_period"] + 1
            frames = sc.frames_of(str(z[name + ".scene"][0]), rows, cols, T, train, seed)
            assert mc.crc(frames) == int(z[name + ".frames_crc"][0]), name
            frames.setflags(write=False)
            counts = z[name + ".counts"]
            ends = np.cumsum(counts)
            boxes, dist = z[name + ".boxes"].astype(np.int32), z[name + ".dist"]
            r = dict(maps(name, (T - train, p["reduced_height"], p["reduced_width"])), params=p, frames=frames, train=train, counts=counts,
                     boxes=[boxes[e - c:e] for c, e in zip(counts, ends)], dist=[dist[e - c:e] for c, e in zip(counts, ends)],
                     images=z[name + ".images"] if name + ".images" in z.files else None, image_crc=[int(v) for v in z[name + ".image_crc"]],
                     plane_crc=dict(zip(mc.STATE_PLANES, (int(v) for v in z[name + ".plane_crc"]))))
            out["step"][name] = r
        _FIXTURE = out
    return _FIXTURE
