"""MOG2 per-frame kernels after the instruction-stream rewrite (kernel_mog2.h: wave-relative addressing with a scalar tile base, the
rejection rule as one compare against s_min, the one-record form of the filter kernel, the straight-line rank scan) at the smallest
shapes where each of those can go wrong.  Everything is compared with the CPU oracle: masks bit for bit every frame, the model state
within 1e-4 (gpu_helpers.check_mog2_state), and at sparse level 4 the summaries' invariants over the whole frame."""
import numpy as np
import pytest

from oracle import pyoracle
from tracking_amd import Engine, capi

from gpu_helpers import *  # noqa: F401,F403
from gpu_helpers import _params, _torch
from test_gpu_00_configs import _mog2_summary_invariants

pytestmark = pytest.mark.gpu


def _sat_like(T, S, H, W, seed):
    """5 grey levels 40 apart, every pixel with its own phase, noise +-2: like the benchmark input, every pixel has five well-separated
    modes and matches another one in every frame."""
    rng = np.random.default_rng(seed)
    base = rng.integers(20, 40, (S, H, W, 3))
    phase = rng.integers(0, 5, (S, H, W, 1))
    frames = np.empty((T, S, H, W, 3), np.uint8)
    for t in range(T):
        frames[t] = (base + 40 * ((t + phase) % 5) + rng.integers(-2, 3, (S, H, W, 3))).astype(np.uint8)
    return frames


@pytest.mark.parametrize("level", [1, 2, 4])
@pytest.mark.parametrize("geometry", [(3, 45, 37), (1, 16, 16)])
def test_waves_that_straddle_tiles_and_streams(level, geometry):
    """n = 45 x 37 = 1 665 pixels per stream is no multiple of 64.  Even frames go through ONE launch over all streams (streams 1 and 2
    then start in the middle of a wave and of a tile, the last wave is partial); odd frames through one launch for stream 0 and one
    for streams 1 .. 2, which starts at model pixel 1 665 - its waves start at 129, 193, ... inside a 256-pixel tile, so every fourth
    wave runs over the end of its tile (the per-lane part of the addressing).  16 x 16 is a single tile."""
    torch = _torch()
    S, H, W = geometry
    T, n = 40, H * W
    frames = _sat_like(T, S, H, W, seed=7 * level + S)
    eng = Engine(capi.MOG2, n_streams=S)
    eng.set_geometry(H, W, 3)
    eng.set_option(capi.OPT_MOG2_SPARSE, level)
    orcs = [pyoracle.Oracle(capi.MOG2) for _ in range(S)]
    d_fg = torch.zeros((S, H, W), dtype=torch.uint8, device="cuda")
    for t in range(T):
        d = torch.from_numpy(frames[t]).cuda()
        if t % 2 == 0 or S == 1:
            assert eng.process_batch_device(d, d_fg, None, None) & capi.FG_VALID
        else:
            assert eng.process_batch_device(d[:1], d_fg[:1], None, None, first=0, count=1) & capi.FG_VALID
            assert eng.process_batch_device(d[1:], d_fg[1:], None, None, first=1, count=S - 1) & capi.FG_VALID
        torch.cuda.synchronize()
        got = d_fg.cpu().numpy()
        for s in range(S):
            ofg, _ = orcs[s].process(frames[t, s], want_bg=False)
            assert np.array_equal(got[s], ofg), (level, t, s, int((got[s] != ofg).sum()))
        if t + 1 in (10, 25, 40):
            for s in range(S):
                check_mog2_state(eng, orcs[s], n, stream=s)
    if level == 4:
        for s in range(S):
            assert _mog2_summary_invariants(eng, n, stream=s) == 1.0
    eng.close()


def _abandoning_walk(T, H, W, seed):
    """Per pixel 2 - 6 grey levels 36 apart; a pixel stays on a level for a while, then leaves it for 15 - 25 frames and visits the
    others meanwhile: abandoned modes decay until their weight crosses -prune while modes of lower rank still exist."""
    rng = np.random.default_rng(seed)
    nlev = rng.integers(2, 7, (H, W))
    base = rng.integers(8, 24, (H, W, 3))
    frames = np.empty((T, H, W, 3), np.uint8)
    cur = rng.integers(0, 6, (H, W)) % nlev
    away = np.zeros((6, H, W), np.int64)  # frames a level stays abandoned
    for t in range(T):
        leave = rng.random((H, W)) < 0.3
        for _ in range(3):  # move to a level that is not serving its absence (a few tries; two-level pixels may stay)
            cand = rng.integers(0, 6, (H, W)) % nlev
            ok = leave & (cand != cur) & (np.take_along_axis(away, cand[None], 0)[0] <= 0)
            gone = np.where(ok, cur, -1)
            for lv in range(6):
                away[lv][gone == lv] = rng.integers(15, 26, int((gone == lv).sum()))
            cur = np.where(ok, cand, cur)
            leave &= ~ok
        away -= 1
        frames[t] = (base + 36 * cur[:, :, None] + rng.integers(-2, 3, (H, W, 3))).astype(np.uint8)
    return frames


@pytest.mark.parametrize("level", [2, 4])
@pytest.mark.parametrize("ct", [0.05, 0.3])
@pytest.mark.parametrize("alpha", [0.05, 0.2, -1.0])
def test_prune_quirk_under_the_straight_line_rank_scan(alpha, ct, level):
    """The reference lowers nmodes INSIDE its mode loop when a weight falls below -prune, so the ranks behind a pruned mode are not even
    decayed in that frame, and restores the count afterwards: the model then holds a zero weight at a rank below nmodes.  The kernel's
    rank scan expresses that with selects.  The inputs are checked to get there: the oracle's own state must show such a weight."""
    torch = _torch()
    H, W, T = 64, 64, 60
    n = H * W
    frames = _abandoning_walk(T, H, W, seed=int(1000 * abs(alpha)) + int(100 * ct))
    p = _params(capi.MOG2, alpha=alpha, mog2_ct=ct)
    eng = Engine(capi.MOG2, params=p)
    eng.set_geometry(H, W, 3)
    eng.set_option(capi.OPT_MOG2_SPARSE, level)
    orc = pyoracle.Oracle(capi.MOG2, params=p)
    d_fg = torch.zeros((1, H, W), dtype=torch.uint8, device="cuda")
    pruned_seen = 0
    for t in range(T):
        assert eng.process_batch_device(torch.from_numpy(frames[t:t + 1]).cuda(), d_fg, None, None) & capi.FG_VALID
        torch.cuda.synchronize()
        ofg, _ = orc.process(frames[t], want_bg=False)
        got = d_fg[0].cpu().numpy()
        assert np.array_equal(got, ofg), (alpha, ct, level, t, int((got != ofg).sum()))
        w, nm = orc.get_state("w", (5, n), np.float32), orc.get_state("nmodes", (n,), np.uint8)
        pruned_seen += int(((w == 0) & (np.arange(5)[:, None] < nm[None, :])).sum())
        if (t + 1) % 10 == 0:
            check_mog2_state(eng, orc, n)
    assert pruned_seen > 0, "the clip never pruned a mode: it does not test what it is for"
    if level == 4:
        assert _mog2_summary_invariants(eng, n) == 1.0
    eng.close()


@pytest.mark.parametrize("thresholds", [(0.0, 0.0), (1e-3, 1e-3), (16.0, 9.0), (4e3, 4e3), (1e9, 1e9)])
def test_threshold_extremes_for_s_min(thresholds):
    """s_min at its ends: thresholds of 0 and 1e-3 (s_min = 4, the smallest distance the rule accepts at all), the defaults 16 / 9,
    4e3 (s_min = 82: hardly anything is ruled out) and 1e9 (the clamp: nothing is).  Modes 6 .. 34 levels apart per column band, as in
    test_mog2_summary_filter_boundary_and_invariants, so that the same comparison is ruled out, barely not, or needs the record."""
    torch = _torch()
    rng = np.random.default_rng(int(thresholds[0]) % 1000 + 5)
    H, W, T = 48, 320, 30
    n = H * W
    spacing = np.repeat(np.array([6, 8, 10, 12, 14, 17, 20, 24, 28, 34]), W // 10)[None, :, None]
    base = rng.integers(10, 60, (H, W, 3))
    phase = rng.integers(0, 5, (H, W, 1))
    p = _params(capi.MOG2, mog2_var_threshold=thresholds[0], mog2_var_threshold_gen=thresholds[1])
    eng = Engine(capi.MOG2, params=p)
    eng.set_geometry(H, W, 3)
    eng.set_option(capi.OPT_MOG2_SPARSE, 4)
    orc = pyoracle.Oracle(capi.MOG2, params=p)
    d_fg = torch.zeros((1, H, W), dtype=torch.uint8, device="cuda")
    for t in range(T):
        lvl = (t + phase) % (3 + t // 10)  # 3, then 4, then 5 levels in play
        f = np.clip(base + spacing * lvl + rng.integers(-3, 4, (H, W, 3)) + t // 12, 0, 255).astype(np.uint8)
        assert eng.process_batch_device(torch.from_numpy(f[None]).cuda(), d_fg, None, None) & capi.FG_VALID
        torch.cuda.synchronize()
        ofg, _ = orc.process(f, want_bg=False)
        got = d_fg[0].cpu().numpy()
        assert np.array_equal(got, ofg), (thresholds, t, int((got != ofg).sum()))
    check_mog2_state(eng, orc, n)
    assert _mog2_summary_invariants(eng, n) == 1.0
    eng.close()
