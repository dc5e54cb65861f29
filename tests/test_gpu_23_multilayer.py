"""MultiLayerBGS (BGS_MULTILAYER, USTC_BGS type 23's class) on the GPU against the outputs of the reference's own
jmo/CMultiLayerBGS.cpp (tests/golden/multilayer_ref.npz, read through tests/multilayer_numpy.py; nothing here needs the reference
tree).  Every comparison is byte for byte: masks, backgrounds, the three state planes, and every other path against the host path.
No tolerance anywhere (DESIGN.md 5.11 names the two places where the contract is the fixture's stand-in)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import multilayer_numpy as ml
import multilayer_scenes as sc
from gpu_helpers import _torch
from tracking_amd import Engine, capi

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ALGO = getattr(capi, "MULTILAYER", None)
BOTH = capi.FG_VALID | capi.BG_VALID


def engine(p, n_streams=1):
    e = Engine(ALGO, n_streams=n_streams)
    e.set_multilayer_params(**{k: p[k] for k in ml.FIELDS})
    return e


def state_of(eng, n, stream=0):
    return {"order": eng.get_state("order", (n, 7), np.uint8, stream=stream), "modes": eng.get_state("modes", (n, 5, 18), np.float32, stream=stream),
            "dist": eng.get_state("dist", (n,), np.float32, stream=stream)}


def same_state(a, b, where):
    for pl in a:
        assert a[pl].tobytes() == b[pl].tobytes(), (where, pl)


def host_run(p, frames):
    """The host path, one stream: masks, backgrounds and the state after the last frame."""
    T, H, W = frames.shape[:3]
    eng = engine(p)
    masks, bgs = np.zeros((T, H, W), np.uint8), np.zeros((T, H, W, 3), np.uint8)
    for t, f in enumerate(frames):
        fg, bg = eng.process(f, want_bg=True)
        assert fg is not None and bg is not None and eng.stream_flags(0) == BOTH  # the first frame hands out the reference's zero mask
        masks[t], bgs[t] = fg, bg
    st = state_of(eng, H * W)
    eng.close()
    masks.setflags(write=False), bgs.setflags(write=False)
    return masks, bgs, st


@functools.lru_cache(maxsize=None)
def single(case):
    """The host path on a fixture case.  Computed once; every other path is compared with it byte for byte."""
    r = ml.load()[case]
    return host_run(r["params"], r["frames"])


@functools.lru_cache(maxsize=None)
def single_clip(gen, rows, cols, T, seed):
    return host_run(dict(ml.DEFAULTS, **ml.FAST), sc.frames_of(gen, rows, cols, T, seed))


def words_of(mask, Wd):
    packed = np.packbits(mask.reshape(-1) != 0, bitorder="little")  # tail bits of the last word zero
    w = np.zeros(Wd * 8, np.uint8)
    w[:len(packed)] = packed
    return w.view(np.uint64)


@pytest.mark.parametrize("case", ml.cases())
def test_host_path_matches_reference_fixture(case):
    r = ml.load()[case]
    masks, bgs, st = single(case)
    bad = [t for t in range(len(masks)) if not np.array_equal(masks[t], r["masks"][t])]
    if bad:  # where to look first: the frame, the pixel, and the final distance map against the fixture's
        t = bad[0]
        where = np.argwhere(masks[t] != r["masks"][t])[0].tolist()
        dd = np.flatnonzero(st["dist"].view(np.uint32) != r["dist"].view(np.uint32))
        assert not bad, (case, "first differing frame", t, "pixel", where, "frames", bad[:5], "dist words differing after the last frame", dd[:5].tolist())
    assert [ml.crc(b) for b in bgs] == [int(c) for c in r["bg_crc"]], case
    assert st["order"].tobytes() == r["order"].tobytes(), (case, int((st["order"] != r["order"]).any(1).sum()))
    assert ml.crc(st["modes"]) == r["modes_crc"], case
    if "modes" in r:
        assert st["modes"].tobytes() == r["modes"].tobytes(), case
    assert st["dist"].tobytes() == r["dist"].tobytes(), (case, int((st["dist"].view(np.uint32) != r["dist"].view(np.uint32)).sum()))


def test_batch_path_streams_joining_late_and_a_reset_equal_their_single_stream_runs():
    """Three streams of 37 x 53 in one engine; stream k joins 2 k steps late, so a launch holds a stream on its first frame beside
    older ones; stream 1 is reset at step 9 and fed its clip again from frame 0.  Masks, backgrounds and packed words (1 961 pixels
    are no multiple of 64) equal each stream's own host run, and so does the final state of stream 0."""
    torch = _torch()
    T, H, W, S = 16, 37, 53, 3
    clips = [("scripted", H, W, T, 41 + s) for s in range(S)]
    runs = [single_clip(*c) for c in clips]
    frames = [sc.frames_of(*c) for c in clips]
    n, Wd = H * W, (H * W + 63) // 64
    eng = engine(dict(ml.DEFAULTS, **ml.FAST), n_streams=S)
    eng.set_geometry(H, W, 3)
    join, start, reset_at, seen255 = (0, 2, 4), [0, 2, 4], 9, 0
    for u in range(T):
        if u == reset_at:
            eng.reset_stream(1)
            start[1] = reset_at
            assert eng.frames_seen(1) == 0 and not eng.get_state("order", (n, 7), np.uint8, stream=1).any()
        k = sum(1 for s in range(S) if join[s] <= u)
        d_frames = torch.from_numpy(np.stack([frames[s][u - start[s]] for s in range(k)])).cuda()
        d_fg = torch.full((k, H, W), 9, dtype=torch.uint8, device="cuda")
        d_bg = torch.full((k, H, W, 3), 9, dtype=torch.uint8, device="cuda")
        d_bits = torch.full((k, Wd), -1, dtype=torch.int64, device="cuda")
        assert eng.process_batch_device(d_frames, d_fg, d_bg, d_bits, first=0, count=k) == BOTH
        torch.cuda.synchronize()
        fg, bg, bits = d_fg.cpu().numpy(), d_bg.cpu().numpy(), d_bits.cpu().numpy().view(np.uint64)
        for s in range(k):
            want, wbg = runs[s][0][u - start[s]], runs[s][1][u - start[s]]
            assert np.array_equal(fg[s], want), (u, s, int((fg[s] != want).sum()))
            assert np.array_equal(bg[s], wbg), (u, s)
            assert np.array_equal(bits[s], words_of(want, Wd)), (u, s)
            seen255 += int((want == 255).sum())
    assert seen255 > 500
    same_state(state_of(eng, n, stream=0), runs[0][2], "stream 0")
    eng.close()


def test_neighbour_reads_and_blur_halo_stay_inside_a_stream_s_image():
    """Two 65 x 131 streams in one launch whose facing borders differ by 200 gray levels: stream 0 ends in bright rows, stream 1
    begins with dark ones.  An LBP neighbour or a blur tap that crossed from one image into the next would change the bits or the
    smoothed distances along those rows; each stream must equal its own single-stream run."""
    torch = _torch()
    T, H, W = 8, 65, 131
    p = dict(ml.DEFAULTS, **ml.FAST)
    clips = []
    for s, (top, bottom) in enumerate(((30, 230), (30, 230))):
        f = sc.frames_of("scripted", H, W, T, 51 + s).astype(np.int64)
        f[:, -6:] = np.clip(f[:, -6:] // 8 + bottom - 16, 0, 255)  # bright last rows
        f[:, :6] = np.clip(f[:, :6] // 8 + top - 16, 0, 255)       # dark first rows
        clips.append(f.astype(np.uint8))
    assert int(clips[0][0, -1].mean()) - int(clips[1][0, 0].mean()) >= 195
    runs = [host_run(p, c) for c in clips]
    eng = engine(p, n_streams=2)
    eng.set_geometry(H, W, 3)
    for t in range(T):
        d_frames = torch.from_numpy(np.stack([clips[0][t], clips[1][t]])).cuda()
        d_fg = torch.full((2, H, W), 9, dtype=torch.uint8, device="cuda")
        d_bg = torch.full((2, H, W, 3), 9, dtype=torch.uint8, device="cuda")
        assert eng.process_batch_device(d_frames, d_fg, d_bg, None) == BOTH
        torch.cuda.synchronize()
        for s in range(2):
            assert np.array_equal(d_fg.cpu().numpy()[s], runs[s][0][t]), (t, s)
            assert np.array_equal(d_bg.cpu().numpy()[s], runs[s][1][t]), (t, s)
    for s in range(2):
        same_state(state_of(eng, H * W, stream=s), runs[s][2], "stream %d" % s)
    eng.close()


@pytest.mark.parametrize("case", ["fast", "detect_after"])
def test_clip_call_equals_frame_by_frame(case):
    """Clips of 1, 2, 3, ... frames to the end, the switch at detect_after inside one call.  Masks, backgrounds, packed words and the
    final state equal the host path's."""
    torch = _torch()
    r = ml.load()[case]
    frames, p = r["frames"], r["params"]
    N, H, W = frames.shape[:3]
    n, Wd = H * W, (H * W + 63) // 64
    want_masks, want_bgs, want_state = single(case)
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
    same_state(state_of(eng, n), want_state, "clip against the host path")
    eng.close()


def test_submit_wait_equals_the_host_path():
    case = "K3"
    r = ml.load()[case]
    frames, p = r["frames"], r["params"]
    H, W = frames.shape[1:3]
    want_masks, want_bgs, want_state = single(case)
    sub = engine(p, n_streams=2)
    lfg, lbg = np.zeros((H, W), np.uint8), np.zeros((H, W, 3), np.uint8)
    for t in range(len(frames)):
        sub.submit(np.ascontiguousarray(frames[t]), lfg, lbg, stream=1)
        assert sub.wait(stream=1) == BOTH
        assert np.array_equal(lfg, want_masks[t]) and np.array_equal(lbg, want_bgs[t]), ("submit", t)
    same_state(state_of(sub, H * W, stream=1), want_state, "submit / wait")
    assert sub.frames_seen(0) == 0
    sub.close()


def test_poisoned_allocations_change_nothing():
    """BGS_DEBUG_POISON=1 fills every fresh device buffer with 0xA5: the engine, in a child process, gives the fixture's bytes."""
    case = "dark"
    r = ml.load()[case]
    code = ("import sys, numpy as np\nsys.path.insert(0, %r)\nimport multilayer_numpy as ml\nfrom tracking_amd import Engine, capi\n"
            "r = ml.load()[%r]\np = r['params']\ne = Engine(capi.MULTILAYER)\ne.set_multilayer_params(**p)\n"
            "out = [e.process(f, want_bg=True) for f in r['frames']]\nn = r['order'].shape[0]\n"
            "print(ml.crc(np.array([o[0] for o in out])), ml.crc(np.array([o[1] for o in out])), ml.crc(e.get_state('modes', (n, 5, 18), np.float32)), ml.crc(e.get_state('order', (n, 7), np.uint8)))\n") % (HERE, case)
    env = dict(os.environ, BGS_DEBUG_POISON="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    masks, bgs, _ = single(case)
    assert np.array_equal(masks, r["masks"])
    assert res.stdout.split() == [str(ml.crc(np.array(masks))), str(ml.crc(np.array(bgs))), str(r["modes_crc"]), str(ml.crc(r["order"]))], res.stdout


def test_parameters_set_after_the_geometry_and_gray_frames():
    r = ml.load()["K3"]
    frames, p = r["frames"], r["params"]
    eng = engine(p)
    with pytest.raises(capi.BgsError) as ei:
        eng.process(np.zeros((12, 16), np.uint8))
    assert ei.value.code == capi.ERR_UNSUPPORTED and ml.CLASS_NAME in str(ei.value)
    for t, f in enumerate(frames):
        if t == 3:
            eng.set_multilayer_params(max_mode_num=5, bg_prob_threshold=0.9, texture_weight=0.0)  # accepted, changes nothing
            with pytest.raises(capi.BgsError):
                eng.set_multilayer_params(max_mode_num=6)
        fg, _ = eng.process(f, want_bg=False)
        assert np.array_equal(fg, single("K3")[0][t]), t
    q = eng.get_multilayer_params()
    assert (q.max_mode_num, q.bg_prob_threshold, q.texture_weight) == (3, float(np.float32(0.2)), 0.5)
    eng.close()
    with pytest.raises(capi.BgsError):
        Engine(capi.VUMETER).set_multilayer_params(max_mode_num=4)
    with pytest.raises(capi.BgsError) as ei:
        from tracking_amd.engine import Group
        Group([capi.MOG2, capi.MULTILAYER])
    assert "not built for class groups" in str(ei.value) and ml.CLASS_NAME in str(ei.value)


def run_demo(tmp_path, frames, xml):
    """bgs_demo with FrameProcessor's enableMultiLayerBGS on `frames`: (stdout, masks, the class's XML after the run)."""
    from test_gpu_01_host_cpp import DEMO, HOST, write_fp_config
    subprocess.run(["make", "-s", "-C", HOST], check=True)
    n, rows, cols = frames.shape[:3]
    name = "MultiLayerBGS"
    wd = tmp_path
    (wd / "config").mkdir(parents=True)
    raw = str(wd / "frames.raw")
    frames.tofile(raw)
    write_fp_config(str(wd / "config"), set())
    path = str(wd / "config" / "FrameProcessor.xml")
    text = open(path).read().replace("</opencv_storage>", "<enableMultiLayerBGS>1</enableMultiLayerBGS>\n</opencv_storage>")
    open(path, "w").write(text)
    if xml:
        (wd / "config" / (name + ".xml")).write_text(xml)
    res = subprocess.run([DEMO, raw, str(rows), str(cols), str(n), str(wd / "out")], cwd=str(wd), capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    got = np.fromfile(str(wd / ("out.%s.raw" % name)), np.uint8).reshape(n, rows, cols)
    return res.stdout, got, (wd / "config" / (name + ".xml")).read_text()


def test_host_class_on_the_fast_clip_equals_the_fixture(tmp_path):
    """The C++ class through bgs_demo with the `fast` parameters in its XML (loadDefaultParams 0): the fixture's masks."""
    r = ml.load()["fast"]
    p = r["params"]
    keys = [k for k in ml.FIELDS if k not in ("status", "disable_detect_mode", "disable_learning", "detect_after")]
    xml = '<?xml version="1.0"?>\n<opencv_storage>\n<loadDefaultParams>0</loadDefaultParams>\n' + "".join("<%s>%s</%s>\n" % (k, repr(p[k]), k) for k in keys) + "</opencv_storage>\n"
    out, got, _ = run_demo(tmp_path, r["frames"], xml)
    assert "MultiLayerBGS()" in out and "~MultiLayerBGS()" in out  # the reference's banners
    assert np.array_equal(got, r["masks"])


def test_host_class_through_frame_processor_with_the_defaults(tmp_path):
    """FrameProcessor with enableMultiLayerBGS and no XML: the loadDefaultParams block, setStatus(MLBGS_LEARN) before every frame,
    the XML the first frame saves."""
    r = ml.load()["defaults"]
    out, got, xml = run_demo(tmp_path, r["frames"], None)
    assert np.array_equal(got, r["masks"])
    assert "<loadDefaultParams>1</loadDefaultParams>" in xml and "<max_mode_num>5</max_mode_num>" in xml and "<detectAfter>0</detectAfter>" in xml
