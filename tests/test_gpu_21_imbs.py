"""IndependentMultimodalBGS (BGS_IMBS, USTC_BGS type 33's class) on the GPU against the outputs of the reference's own db/imbs.cpp
(tests/golden/imbs_ref.npz, read through tests/imbs_numpy.py; nothing here needs the reference tree).  The model is integer, the HSV
test is the reference's float sequence and the area filter counts in integers: every comparison here is byte for byte - masks,
backgrounds, the control scalars, the state planes, and every other path against the host path."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import imbs_numpy as im
from gpu_helpers import _torch
from tracking_amd import Engine, capi

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ALGO = getattr(capi, "IMBS", None)
BOTH = capi.FG_VALID | capi.BG_VALID
PKEYS = tuple(im.DEFAULTS)


def engine(p, n_streams=1):
    e = Engine(ALGO, n_streams=n_streams)
    e.set_imbs_params(**{k: p[k] for k in PKEYS})
    return e


def state_of(eng, p, n, stream=0):
    cap, M = p["numSamples"], p["numSamples"] // p["minBinHeight"]
    return {"bins": eng.get_state("bins", (n, cap, 5), np.uint8, stream=stream), "model": eng.get_state("model", (n, M, 6), np.uint8, stream=stream),
            "persistence": eng.get_state("persistence", (n,), np.uint32, stream=stream), "control": eng.get_state("control", (len(im.CONTROL),), np.float64, stream=stream)}


def same_state(a, b, where):
    for pl in a:
        assert a[pl].tobytes() == b[pl].tobytes(), (where, pl)


@functools.lru_cache(maxsize=None)
def single(case):
    """The host path on a fixture case, one stream: masks, backgrounds, the control scalars after every frame and the state after
    the last one.  Computed once; every other path is compared with it byte for byte."""
    r = im.load()[case]
    frames, p = r["frames"], r["params"]
    T, H, W = frames.shape[:3]
    eng = engine(p)
    masks, bgs, ctl = np.zeros((T, H, W), np.uint8), np.zeros((T, H, W, 3), np.uint8), np.zeros((T, len(im.CONTROL)))
    for t, f in enumerate(frames):
        fg, bg = eng.process(f, want_bg=True)
        assert fg is not None and bg is not None and eng.stream_flags(0) == BOTH  # the learning phase hands out valid zero images
        masks[t], bgs[t] = fg, bg
        ctl[t] = eng.get_state("control", (len(im.CONTROL),), np.float64)
    st = state_of(eng, p, H * W)
    eng.close()
    for a in (masks, bgs, ctl):
        a.setflags(write=False)
    return masks, bgs, ctl, st


def words_of(mask, Wd):
    packed = np.packbits(mask.reshape(-1) != 0, bitorder="little")  # tail bits of the last word zero
    w = np.zeros(Wd * 8, np.uint8)
    w[:len(packed)] = packed
    return w.view(np.uint64)


@pytest.mark.parametrize("case", list(im.cases()))
def test_host_path_matches_reference_fixture(case):
    r = im.load()[case]
    masks, bgs, ctl, st = single(case)
    bad = [t for t in range(len(masks)) if not np.array_equal(masks[t], r["masks"][t])]
    assert not bad, (case, bad[:5], int((masks[bad[0]] != r["masks"][bad[0]]).sum()))
    assert [im.crc(b) for b in bgs] == [int(c) for c in r["bg_crc"]], case
    assert ctl.tobytes() == r["control"].tobytes(), (case, [t for t in range(len(ctl)) if ctl[t].tobytes() != r["control"][t].tobytes()][:3])
    assert st["control"].tobytes() == r["control"][-1].tobytes()
    for pl in ("bins", "model", "persistence"):
        if pl in r:
            assert st[pl].tobytes() == r[pl].tobytes(), (case, pl, int((st[pl] != r[pl]).sum()))


def test_batch_path_streams_joining_late_and_a_reset_equal_their_single_stream_runs():
    """Three streams of 37 x 53 in one engine; stream k joins 2 k steps late, so a launch holds a stream on its first frame beside
    sampling, building and detecting ones; stream 1 is reset at step 9 and fed its clip again from frame 0.  Masks, backgrounds and
    packed words (made from the byte masks: 1 961 pixels are no multiple of 64) equal each stream's own host run, and so does the
    final state of stream 0."""
    torch = _torch()
    cases = ("ragged", "ragged_o1", "ragged_o2")
    rs = [im.load()[c] for c in cases]
    T, H, W = rs[0]["masks"].shape
    n, Wd, S = H * W, (H * W + 63) // 64, 3
    p = rs[0]["params"]
    eng = engine(p, n_streams=S)
    eng.set_geometry(H, W, 3)
    join, start, reset_at, seen255 = (0, 2, 4), [0, 2, 4], 9, 0
    for u in range(T):
        if u == reset_at:
            eng.reset_stream(1)
            start[1] = reset_at
            assert eng.frames_seen(1) == 0 and not eng.get_state("model", (n, 3, 6), np.uint8, stream=1).any()
        k = sum(1 for s in range(S) if join[s] <= u)
        d_frames = torch.from_numpy(np.stack([rs[s]["frames"][u - start[s]] for s in range(k)])).cuda()
        d_fg = torch.full((k, H, W), 9, dtype=torch.uint8, device="cuda")
        d_bg = torch.full((k, H, W, 3), 9, dtype=torch.uint8, device="cuda")
        d_bits = torch.full((k, Wd), -1, dtype=torch.int64, device="cuda")
        assert eng.process_batch_device(d_frames, d_fg, d_bg, d_bits, first=0, count=k) == BOTH
        torch.cuda.synchronize()
        fg, bg, bits = d_fg.cpu().numpy(), d_bg.cpu().numpy(), d_bits.cpu().numpy().view(np.uint64)
        for s in range(k):
            want, wbg = single(cases[s])[0][u - start[s]], single(cases[s])[1][u - start[s]]
            assert np.array_equal(fg[s], want), (u, s, int((fg[s] != want).sum()))
            assert np.array_equal(bg[s], wbg), (u, s)
            assert np.array_equal(bits[s], words_of(want, Wd)), (u, s)
            seen255 += int((want == 255).sum())
    assert seen255 > 500
    same_state(state_of(eng, p, n, stream=0), single("ragged")[3], "stream 0")
    eng.close()


@pytest.mark.parametrize("shape", [(16, 64), (10, 13)])
def test_packed_only_engine_equals_byte_mask_engine(shape):
    """16 x 64 (words straight from the finished byte mask in the engine's own buffer) and 10 x 13 (ragged words)."""
    torch = _torch()
    H, W = shape
    p = dict(im.DEFAULTS, minArea=4.0, **im.FAST)
    frames = im.clip("persist", 20, H, W, 21)
    Wd = (H * W + 63) // 64
    a, b = engine(p), engine(p)
    a.set_geometry(H, W, 3), b.set_geometry(H, W, 3)
    seen = 0
    for f in frames:
        d = torch.from_numpy(f).cuda().unsqueeze(0)
        d_fg = torch.full((1, H, W), 9, dtype=torch.uint8, device="cuda")
        d_bits = torch.full((1, Wd), -1, dtype=torch.int64, device="cuda")
        assert a.process_batch_device(d, d_fg, None, None) == BOTH
        assert b.process_batch_device(d, None, None, d_bits) == BOTH
        torch.cuda.synchronize()
        fg = d_fg.cpu().numpy()[0]
        assert np.array_equal(d_bits.cpu().numpy().view(np.uint64)[0], words_of(fg, Wd))
        seen += int((fg != 0).sum())
    assert seen > 50
    a.close(), b.close()


@pytest.mark.parametrize("case", ["tile", "holes_a2"])
def test_clip_call_equals_frame_by_frame(case):
    """Clips of 1, 2, 3, ... frames to the end: sampling frames, builds and detecting frames inside one call.  Masks, backgrounds,
    packed words and the final state equal the host path's."""
    torch = _torch()
    r = im.load()[case]
    frames, p = r["frames"], r["params"]
    N, H, W = frames.shape[:3]
    n, Wd = H * W, (H * W + 63) // 64
    want_masks, want_bgs, _, want_state = single(case)
    d_all = torch.from_numpy(np.array(frames)).cuda().unsqueeze(1)  # [N][1][H][W][3]
    eng = engine(p)
    eng.set_geometry(H, W, 3)
    t, k = 0, 1
    while t < N:
        k = min(k, N - t)
        d_fg = torch.full((k, 1, H, W), 9, dtype=torch.uint8, device="cuda")
        d_bg = torch.full((k, 1, H, W, 3), 9, dtype=torch.uint8, device="cuda")
        d_bits = torch.full((k, 1, Wd), -1, dtype=torch.int64, device="cuda")
        assert eng.process_clip_device(d_all[t:t + k], k, d_fg, d_bg, d_bits) == [BOTH] * k
        torch.cuda.synchronize()
        assert np.array_equal(d_fg.cpu().numpy()[:, 0], want_masks[t:t + k]), t
        assert np.array_equal(d_bg.cpu().numpy()[:, 0], want_bgs[t:t + k]), t
        bits = d_bits.cpu().numpy().view(np.uint64)[:, 0]
        for i in range(k):
            assert np.array_equal(bits[i], words_of(want_masks[t + i], Wd)), t + i
        t, k = t + k, k + 1
    same_state(state_of(eng, p, n), want_state, "clip against the host path")
    eng.close()


def test_two_ranges_on_two_hip_streams_and_submit_wait_equal_the_host_path():
    torch = _torch()
    case = "sudden"
    r = im.load()[case]
    frames, p = r["frames"], r["params"]
    N, H, W = frames.shape[:3]
    n = H * W
    want_masks, want_bgs, _, want_state = single(case)
    S = 4
    eng, sub = engine(p, n_streams=S), engine(p, n_streams=2)
    eng.set_geometry(H, W, 3)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    lfg, lbg = np.zeros((H, W), np.uint8), np.zeros((H, W, 3), np.uint8)
    for t in range(N):
        d = torch.from_numpy(np.stack([frames[t]] * S)).cuda()
        d_fg = torch.full((S, H, W), 9, dtype=torch.uint8, device="cuda")
        d_bg = torch.full((S, H, W, 3), 9, dtype=torch.uint8, device="cuda")
        torch.cuda.current_stream().synchronize()
        eng.process_batch_device(d[:1], d_fg[:1], d_bg[:1], None, hip_stream=s1.cuda_stream, first=0, count=1)
        eng.process_batch_device(d[1:], d_fg[1:], d_bg[1:], None, hip_stream=s2.cuda_stream, first=1, count=3)
        s1.synchronize(), s2.synchronize()
        fg, bg = d_fg.cpu().numpy(), d_bg.cpu().numpy()
        for s in range(S):
            assert np.array_equal(fg[s], want_masks[t]) and np.array_equal(bg[s], want_bgs[t]), (t, s)
        sub.submit(np.ascontiguousarray(frames[t]), lfg, lbg, stream=1)
        assert sub.wait(stream=1) == BOTH
        assert np.array_equal(lfg, want_masks[t]) and np.array_equal(lbg, want_bgs[t]), ("submit", t)
    for s in (0, 3):
        same_state(state_of(eng, p, n, stream=s), want_state, "range, stream %d" % s)
    same_state(state_of(sub, p, n, stream=1), want_state, "submit / wait")
    assert sub.frames_seen(0) == 0
    eng.close(), sub.close()


@pytest.mark.parametrize("case", ["holes_a2", "sudden"])
def test_poisoned_allocations_change_nothing(case):
    """BGS_DEBUG_POISON=1 fills every fresh device buffer with 0xA5: the engine, in a child process, gives the fixture's bytes."""
    r = im.load()[case]
    code = ("import sys, numpy as np\nsys.path.insert(0, %r)\nimport imbs_numpy as im\nfrom tracking_amd import Engine, capi\n"
            "r = im.load()[%r]\np = r['params']\ne = Engine(capi.IMBS)\ne.set_imbs_params(**{k: p[k] for k in im.DEFAULTS})\n"
            "out = [e.process(f, want_bg=True) for f in r['frames']]\n"
            "print(im.crc(np.array([o[0] for o in out])), im.crc(np.array([o[1] for o in out])), im.crc(e.get_state('model', r['model'].shape, np.uint8)))\n") % (HERE, case)
    env = dict(os.environ, BGS_DEBUG_POISON="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    masks, bgs, _, _ = single(case)
    assert np.array_equal(masks, r["masks"])
    assert res.stdout.split() == [str(im.crc(np.array(masks))), str(im.crc(np.array(bgs))), str(im.crc(r["model"]))], res.stdout


def test_parameters_set_after_the_geometry_and_gray_frames():
    r = im.load()["basic"]
    frames, p = r["frames"], r["params"]
    eng = engine(p)
    with pytest.raises(capi.BgsError) as ei:
        eng.process(np.zeros((12, 16), np.uint8))
    assert ei.value.code == capi.ERR_UNSUPPORTED and im.CLASS_NAME in str(ei.value)
    for t, f in enumerate(frames):
        if t == 3:
            eng.set_imbs_params(numSamples=9, fgThreshold=1, minArea=0.0)  # accepted, changes nothing
            with pytest.raises(capi.BgsError):
                eng.set_imbs_params(numSamples=64)
        fg, _ = eng.process(f, want_bg=False)
        assert np.array_equal(fg, single("basic")[0][t]), t
    q = eng.get_imbs_params()
    assert (q.numSamples, q.fgThreshold, q.minArea) == (p["numSamples"], p["fgThreshold"], p["minArea"])
    eng.close()
    with pytest.raises(capi.BgsError):
        Engine(capi.VUMETER).set_imbs_params(numSamples=4)


def run_demo(tmp_path, frames):
    """bgs_demo with FrameProcessor's enableIMBS on `frames`: (stdout, masks, the class's XML)."""
    from test_gpu_01_host_cpp import DEMO, HOST, write_fp_config
    subprocess.run(["make", "-s", "-C", HOST], check=True)
    n, rows, cols = frames.shape[:3]
    name = "IndependentMultimodalBGS"
    wd = tmp_path
    (wd / "config").mkdir(parents=True)
    raw = str(wd / "frames.raw")
    frames.tofile(raw)
    write_fp_config(str(wd / "config"), set())
    path = str(wd / "config" / "FrameProcessor.xml")
    text = open(path).read().replace("</opencv_storage>", "<enableIMBS>1</enableIMBS>\n</opencv_storage>")
    open(path, "w").write(text)
    res = subprocess.run([DEMO, raw, str(rows), str(cols), str(n), str(wd / "out")], cwd=str(wd), capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    got = np.fromfile(str(wd / ("out.%s.raw" % name)), np.uint8).reshape(n, rows, cols)
    return res.stdout, got, (wd / "config" / (name + ".xml")).read_text()


def test_host_class_through_frame_processor(tmp_path):
    """The C++ host layer on the `default_short` clip: banners, the XML with showOutput alone, and the fixture's masks of the
    learning phase."""
    r = im.load()["default_short"]
    name = "IndependentMultimodalBGS"
    out, got, xml = run_demo(tmp_path, r["frames"])
    assert name + "()" in out and "~" + name + "()" in out  # the reference's banners
    assert np.array_equal(got, r["masks"]) and np.array_equal(got, single("default_short")[0])
    assert xml == '<?xml version="1.0"?>\n<opencv_storage>\n<showOutput>1</showOutput>\n</opencv_storage>\n'


def test_host_class_detects_after_the_first_model_of_the_defaults(tmp_path):
    """The class has no parameter in its XML, so the wrapper's defaults are all it can run: 165 frames of 24 x 32, the first model at
    frame 145, an object that enters at frame 147.  The masks the C++ class writes equal the engine's through the Python binding and
    the restatement's, and they hold foreground."""
    frames = im.clip("late", 165, 24, 32, 31)
    want, _, ctl, _ = im.run(dict(im.DEFAULTS), frames)
    assert int(ctl[:, 9].argmax()) == 145 and not want[:147].any() and all((m == 255).sum() >= 60 for m in want[147:])
    eng = engine(dict(im.DEFAULTS))
    py = np.array([eng.process(f, want_bg=False)[0] for f in frames])
    bg = eng.process(frames[-1], want_bg=True)[1]
    eng.close()
    assert np.array_equal(py, want)
    assert bg.any()  # the background of the build, no banner
    _, got, _ = run_demo(tmp_path, frames)
    bad = [t for t in range(len(got)) if not np.array_equal(got[t], want[t])]
    assert not bad, bad[:5]
