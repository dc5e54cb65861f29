"""DPPratiMediodBGS / DPTextureBGS (BGS_DP_PRATI_MEDIOD, BGS_DP_TEXTURE) on the CPU: the numpy restatement (tests/dp2_numpy.py)
against the outputs of the reference's own code (tests/golden/dp2_ref_*.npz: pinned), the dist invariant, the r-update arithmetic,
the C ABI defaults, the refused parameters and the host class list."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import dp2_numpy as dn
from tracking_amd import capi

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
PRATI_CASES = ["default", "h4_r1", "h1_r3", "thr10", "ties", "ties_h64", "frames96"]
TEXTURE_CASES = ["crop48x80", "crop32x64", "box32x48"]


def _clip(name):
    if name == "frames_96x80":
        return np.load(os.path.join(GOLDEN, "frames_96x80.npz"))["frames"]
    kind, T, H, W, seed = name.split(":")
    return getattr(dn, kind)(int(T), int(H), int(W), int(seed))


def golden(cls, case):
    """(record, params, input frames) of one fixture case; the input is checked against the CRC-32 it was made from."""
    z = np.load(os.path.join(GOLDEN, "dp2_ref_%s.npz" % cls))
    r = {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(case + "/")}
    p = json.loads(str(r["params"]))
    frames = _clip(p["input"])
    if p.get("crop"):
        y0, y1, x0, x1 = p["crop"]
        frames = np.ascontiguousarray(frames[:, y0:y1, x0:x1])
    assert dn.crc(frames) == int(r["input_crc32"]), "%s: input clip differs from the one the fixture was made from" % case
    return r, p, frames


def masks_of(r):
    T, rows, cols = (int(v) for v in r["shape"])
    return np.unpackbits(r["masks"], axis=-1)[..., :cols].reshape(T, rows, cols) * np.uint8(255)


def prati_kwargs(p):
    return {k: p[k] for k in ("threshold", "sampling_rate", "history_size")}


def run_prati(frames, **kw):
    m = dn.Prati(**kw)
    return m, np.array([m.process(f) for f in frames])


@pytest.mark.parametrize("case", PRATI_CASES)
def test_prati_restatement_matches_reference_fixture(case):
    r, p, frames = golden("prati", case)
    m, got = run_prati(frames, **prati_kwargs(p))
    want = masks_of(r)
    bad = np.nonzero((got != want).reshape(len(got), -1).any(1))[0]
    assert not len(bad), "%s: frames %s differ" % (case, bad[:5])
    assert (want[:p["history_size"]] == 0).all()  # Subtract clears the masks while frame_num < historySize
    if "samples" in r:  # the whole model after the last frame
        for name, v in m.planes().items():
            assert np.array_equal(v, r[name]), name
        assert (m.cnt, m.pos) == tuple(int(v) for v in r["count"])


def test_prati_fixtures_cover_what_they_claim():
    r, p, frames = golden("prati", "default")
    assert len(frames) >= 120 and (p["sampling_rate"], p["history_size"], p["threshold"]) == (5, 16, 30)
    assert int(r["count"][0]) == 16 and masks_of(r)[80:].any()  # the buffer wrapped and the masks are not trivial
    r, p, frames = golden("prati", "ties")
    assert set(np.unique(frames)) <= {0, 128, 255}


@pytest.mark.parametrize("H,rate,seed", [(64, 1, 1), (64, 2, 2), (16, 1, 3), (5, 3, 4)])
def test_prati_dist_invariant_on_adversarial_clips(H, rate, seed):
    """Every dist entry is a sum of at most historySize L-inf terms of at most 255 each and never negative - so it fits uint16 for
    historySize <= 64.  Saturated clips that alternate 0 / 255 push the sums to their ceiling."""
    rng = np.random.default_rng(seed)
    T = H * rate + 3 * H
    frames = np.where(rng.random((T, 4, 5, 1)) < 0.5, 0, 255).astype(np.uint8).repeat(3, -1)
    frames[::7] = dn.tie_clip(len(frames[::7]), 4, 5, seed)
    m = dn.Prati(history_size=H, sampling_rate=rate, threshold=0)
    peak = 0
    for f in frames:
        m.process(f)
        d = m.dist[:m.cnt]
        assert (d >= 0).all() and (d <= H * 255).all()
        peak = max(peak, int(d.max(initial=0)))
    assert peak > (H - 1) * 255 * 0.4


def test_r_update_integer_form_equals_the_double_expression():
    """The kernel's bg + floor((13421773 (cur - bg) + 2^27) / 2^28) equals (unsigned char)(ALPHA*cur + (1-ALPHA)*bg + 0.5) with
    ALPHA = 0.05f widened to double, for every (cur, bg) byte pair (cur only reaches 121 in the interior)."""
    cur, bg = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    want = dn.r_update(cur, bg)
    assert dn.ALPHA == 13421773 / 2 ** 28
    got = bg + ((13421773 * (cur - bg) + (1 << 27)) >> 28)
    assert np.array_equal(got, want)
    # and the same through Python's own scalar doubles (no vectorised path involved)
    for c in range(0, 256, 5):
        for b in range(256):
            assert int(dn.ALPHA * c + (1 - dn.ALPHA) * b + 0.5) == want[c, b]


@pytest.mark.parametrize("case", TEXTURE_CASES)
def test_texture_restatement_matches_reference_fixture(case):
    r, p, frames = golden("texture", case)
    m = dn.Texture()
    got = np.array([m.process(f) for f in frames])
    want = masks_of(r)
    bad = np.nonzero((got != want).reshape(len(got), -1).any(1))[0]
    assert not len(bad), "%s: frames %s differ" % (case, bad[:5])
    if "hist_interior" in r:
        T, H, W = (int(v) for v in r["shape"])
        hist = m.hist_plane().reshape(H, W, 3, 64)
        e = dn.EDGE
        assert np.array_equal(hist[e:H - e, e:W - e], r["hist_interior"])
        assert not hist[:e].any() and not hist[:, :e].any()


def test_texture_only_r_moves_and_fixture_geometries_are_defined():
    r, p, frames = golden("texture", "box32x48")
    T, H, W = (int(v) for v in r["shape"])
    e = dn.EDGE
    ys, xs = np.mgrid[e:H - e, e:W - e]
    first = dn.histograms(dn.lbp(frames[0]), ys.ravel(), xs.ravel()).reshape(H - 2 * e, W - 2 * e, 3, 64)
    h = r["hist_interior"]
    assert np.array_equal(h[..., 1:, :], first[..., 1:, :])  # g and b keep the first frame's histograms
    assert not np.array_equal(h[..., 0, :], first[..., 0, :])  # r adapts
    assert masks_of(r).any()
    for case in TEXTURE_CASES:
        T, H, W = (int(v) for v in golden("texture", case)[0]["shape"])
        assert W % 4 == 0 and (W - 8) * W + (H - 8) < H * W  # every fgMask(x, y) read of the reference is defined


def test_texture_gate_rule():
    """fgMask(x, y): flat byte x * widthStep + y; past the image or in row padding -> -1 (reads as 0)."""
    g = dn.gate_source(20, 30, np.array([7, 9]), np.array([8, 22]))  # portrait-ish rows 20, cols 30 (ws 32)
    assert g.tolist() == [8 * 30 + 7, -1]  # (y 9, x 22): flat 22 * 32 + 9 = 713 -> row 22 >= 20
    g = dn.gate_source(40, 30, np.array([31 - 1]), np.array([7]))  # ws 32: flat 7 * 32 + 30 -> column 30 of row 7 is padding
    assert g.tolist() == [-1]


def test_small_frames_give_empty_masks():
    f = np.random.default_rng(0).integers(0, 256, (6, 14, 14, 3), dtype=np.uint8)
    m = dn.Texture()
    assert not any(m.process(x).any() for x in f)
    m = dn.Prati(history_size=1, sampling_rate=1, threshold=0)
    assert not any(m.process(x[:2, :2]).any() for x in f)


def test_default_params_hold_the_reference_defaults():
    assert (capi.DP_PRATI_MEDIOD, capi.DP_TEXTURE) == (19, 20)
    p = capi.default_params(capi.DP_PRATI_MEDIOD)
    assert (p.dp_threshold, p.dp_sampling_rate, p.dp_history_size, p.dp_weight) == (30.0, 5, 16, 5)  # DPPratiMediodBGS.cpp:19
    for algo in range(19):
        q = capi.default_params(algo)
        assert (q.dp_history_size, q.dp_weight) == (0, 0), algo
        assert (q.kde_frames_to_learn != 0) == (algo == capi.KDE)
    q = capi.default_params(capi.DP_TEXTURE)
    assert (q.dp_history_size, q.dp_weight, q.kde_sequence_length) == (0, 0, 0)
    assert capi.lib().bgs_abi_version() == 1


def test_params_struct_tail_matches_c(tmp_path):
    inc = os.path.join(HERE, os.pardir, "include")
    src = tmp_path / "dp2_sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bgs_hip.h"\nint main(){printf("%zu %zu %zu %d %d %d %d\\n", sizeof(bgs_params), '
                   'offsetof(bgs_params, dp_history_size), offsetof(bgs_params, dp_weight), (int)BGS_DP_PRATI_MEDIOD, (int)BGS_DP_TEXTURE, '
                   '(int)BGS_ALGO_COUNT, BGS_PRATI_MAX_HISTORY);return 0;}\n')
    exe = tmp_path / "dp2_sz"
    subprocess.run(["gcc", "-I", inc, str(src), "-o", str(exe)], check=True)
    size, a, b, pm, tx, count, hmax = map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split())
    assert size == C.sizeof(capi.BgsParams) and (pm, tx, count) == (capi.DP_PRATI_MEDIOD, capi.DP_TEXTURE, 21)
    assert a == capi.BgsParams.dp_history_size.offset and b == capi.BgsParams.dp_weight.offset
    assert a > capi.BgsParams.kde_alpha.offset and hmax == capi.PRATI_MAX_HISTORY == 64


@pytest.mark.parametrize("field,value", [("dp_sampling_rate", 0), ("dp_history_size", 0), ("dp_history_size", -3),
                                         ("dp_history_size", 65), ("dp_threshold", -1.0), ("dp_threshold", float("nan"))])
def test_refused_parameters(field, value):
    p = capi.default_params(capi.DP_PRATI_MEDIOD)
    setattr(p, field, value)
    h = C.c_void_p()
    assert capi.lib().bgs_create(capi.DP_PRATI_MEDIOD, C.byref(p), 0, 1, C.byref(h)) == capi.ERR_UNSUPPORTED
    assert b"PratiMediod" in capi.lib().bgs_last_error()
