"""The frame generators behind tests/golden/multilayer_ref.npz: the fixture stores a generator's name, its size, frame count and
seed, and the CRC of the frames it made (numpy's legacy RandomState is stable across versions)."""
import numpy as np


def _texture(rs, rows, cols, lo, hi):
    """a blocky BGR texture, so that the six LBP neighbours at radius 2 differ by more than the noise offset in many places"""
    small = rs.randint(lo, hi, (rows // 3 + 2, cols // 3 + 2, 3))
    return np.kron(small, np.ones((3, 3, 1), np.int64))[:rows, :cols].astype(np.int64)


def _noisy(rs, img, amp):
    return np.clip(img + rs.randint(-amp, amp + 1, img.shape), 0, 255).astype(np.uint8)


def static_block(rows, cols, T, seed):
    """a static textured scene with sensor noise and a bright block moving two pixels a frame"""
    rs = np.random.RandomState(seed)
    base = _texture(rs, rows, cols, 40, 200)
    out = []
    for t in range(T):
        f = _noisy(rs, base, 2)
        y, x = (3 + t) % max(rows - 8, 1), (2 * t) % max(cols - 8, 1)
        f[y:y + 8, x:x + 8] = _noisy(rs, np.full((min(8, rows - y), min(8, cols - x), 3), 230), 3)
        out.append(f)
    return np.stack(out)


def scripted(rows, cols, T, seed):
    """scene A for 6 frames, B for 5, A for 3, then C; columns 0-5 are fresh noise in every frame (modes fill up and are replaced),
    columns 6-11 show noise in B's last frame (a removal in front of the matched mode), and the top rows change to D for the last
    four frames (a freed slot is used again)"""
    rs = np.random.RandomState(seed)
    A, B, C, D = _texture(rs, rows, cols, 30, 90), _texture(rs, rows, cols, 110, 170), _texture(rs, rows, cols, 190, 250), _texture(rs, rows, cols, 60, 220)
    out = []
    for t in range(T):
        scene = A if t < 6 else B if t < 11 else A if t < 14 else C
        f = _noisy(rs, scene, 1)
        f[:, :min(6, cols)] = rs.randint(0, 256, f[:, :min(6, cols)].shape)
        if t == 10:
            f[:, 6:12] = rs.randint(0, 256, f[:, 6:12].shape)
        if t >= T - 4 and t >= 14:
            f[:min(8, rows)] = _noisy(rs, D[:min(8, rows)], 1)
        out.append(f)
    return np.stack(out)


def dark(rows, cols, T, seed):
    """4 x 4 blocks that hold black, near-black, mid and saturated levels and jump between them: the zero norm, the ratio >= 1 and
    the shadow / highlight limits"""
    rs = np.random.RandomState(seed)
    levels = np.array([0, 0, 1, 2, 3, 5, 8, 60, 140, 150, 200, 215, 255, 255])
    out = []
    cur = rs.randint(0, len(levels), (rows // 4 + 1, cols // 4 + 1, 1))  # one level for the three channels of a block
    for t in range(T):
        jump = rs.randint(0, 3, cur.shape[:2]) == 0
        cur = np.where(jump[..., None], rs.randint(0, len(levels), cur.shape), cur)
        f = np.kron(np.repeat(levels[cur], 3, 2), np.ones((4, 4, 1), np.int64))[:rows, :cols]
        out.append(np.clip(f + (rs.randint(0, 2, f.shape) if t % 3 == 2 else 0), 0, 255).astype(np.uint8))
    return np.stack(out)


def scaled_block(rows, cols, T, seed):
    """static_block's scene with a block of a third of the frame each way (at least one pixel) that moves half its size a frame: a
    frame of any size shows foreground and background.  The first five frames show another scene, which never comes back: with fast
    rates its mode becomes a layer and then decays until the first form of the layer removal takes it, 14 frames later.  Not in the reference fixture; the models fuzz draws it."""
    rs = np.random.RandomState(seed)
    first, base = _texture(rs, rows, cols, 140, 250), _texture(rs, rows, cols, 40, 120)
    bh, bw = max(rows // 3, 1), max(cols // 3, 1)
    out = []
    for t in range(T):
        f = _noisy(rs, first if t < 5 else base, 2)
        y, x = (t * max(bh // 2, 1)) % (rows - bh + 1), (t * max(bw // 2, 1)) % (cols - bw + 1)
        f[y:y + bh, x:x + bw] = _noisy(rs, np.full((bh, bw, 3), 230), 3)
        out.append(f)
    return np.stack(out)


GENERATORS = {"static_block": static_block, "scripted": scripted, "dark": dark, "scaled_block": scaled_block}


def frames_of(gen, rows, cols, T, seed):
    return GENERATORS[str(gen)](int(rows), int(cols), int(T), int(seed))
