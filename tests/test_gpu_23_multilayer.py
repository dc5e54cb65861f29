"""MultiLayerBGS (BGS_MULTILAYER, USTC_BGS type 23's class) on the GPU against the outputs of the reference's own
jmo/CMultiLayerBGS.cpp (tests/golden/multilayer_ref.npz, read through tests/multilayer_numpy.py; nothing here needs the reference
tree), and - at half sizes, launch keys and an emptied mode list the fixture does not hold - against the restatement, which
tests/test_multilayer_cpu.py pins to the reference's code there.  Every comparison is byte for byte: masks, backgrounds, the three
state planes, and every other path against the host path.
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


def test_every_half_size_at_the_smoothing_tile_s_edges():
    """pattern_neig_half_size 1..8 with a narrow and a wide Gaussian on frames of one pixel, one row, and one pixel past, one pixel
    short of and two tiles across the 32 x 8 smoothing tile, all smaller than the largest halo in at least one direction.  Masks,
    backgrounds and the smoothed distance plane equal the restatement's bit for bit, and every half size changes the plane against
    the half size below it somewhere, so a kernel that ignored it could not pass."""
    T, bits = 12, int(ml.load()["defaults"]["consts"][0])
    differs = dict.fromkeys(range(1, 9), False)
    for g, (H, W) in enumerate(((1, 1), (1, 40), (9, 33), (17, 31), (7, 65))):
        frames = sc.frames_of("scripted", H, W, T, 61 + g)
        for sigma in (0.5, 3.0):
            below = ml.run(dict(ml.DEFAULTS, **ml.FAST, pattern_neig_half_size=0, pattern_neig_gaus_sigma=sigma), frames, bits)[0].state()[2]
            for h in range(1, 9):
                p = dict(ml.DEFAULTS, **ml.FAST, pattern_neig_half_size=h, pattern_neig_gaus_sigma=sigma)
                m, want_masks, want_bgs = ml.run(p, frames, bits)
                masks, bgs, st = host_run(p, frames)
                where = (H, W, sigma, h)
                assert np.array_equal(masks, want_masks), (where, int((masks != want_masks).sum()))
                assert np.array_equal(bgs, want_bgs), where
                want = m.state()[2]
                assert st["dist"].tobytes() == want.tobytes(), (where, int((st["dist"].view(np.uint32) != want.view(np.uint32)).sum()))
                differs[h] = differs[h] or st["dist"].tobytes() != below.tobytes()
                below = st["dist"]
    assert all(differs.values()), differs


EMPTIED = dict(dict(ml.DEFAULTS, **ml.FAST), weight_updating_constant=5.0, max_mode_num=4, pattern_neig_half_size=2, bg_prob_threshold=0.1, bg_prob_updating_threshold=0.35,
               min_noised_angle=0.05, shadow_rate=0.4, highlight_rate=2.0)


def test_a_frame_that_empties_the_last_pixel_s_list_is_a_first_frame():
    """weight_updating_constant 5 with a weight rate of 0.5 a frame drives weights below zero; a layered mode below 1e-4 is removed
    even when it is the list's only one, and when that happens to the last pixel the reference's bFirstFrame is true again: a zero
    mask and a zero distance map in the middle of a stream (the models fuzz found it at seed 715035)."""
    frames = sc.frames_of("dark", 9, 33, 8, 5005245)
    m, want_masks, want_bgs = ml.run(EMPTIED, frames, int(ml.load()["defaults"]["consts"][0]))
    assert want_masks[3].any() and not want_masks[4].any() and want_masks[5].any()  # frame 4 is the one
    masks, bgs, st = host_run(EMPTIED, frames)
    assert [t for t in range(len(frames)) if not np.array_equal(masks[t], want_masks[t])] == []
    assert np.array_equal(bgs, want_bgs)
    for pl, want in zip(("order", "modes", "dist"), m.state()):
        assert st[pl].tobytes() == want.tobytes(), pl
    # and the frame's zero map is what the state plane holds right after it
    eng = engine(EMPTIED)
    for f in frames[:5]:
        eng.process(f)
    assert not eng.get_state("dist", (9 * 33,), np.float32).any()
    eng.close()


def test_one_call_holds_first_learning_and_detecting_streams():
    """Three 16 x 33 streams with detect_after 4 join at steps 0, 3 and 6, and stream 0 is reset at step 8 and fed its clip again: the
    calls at steps 6 and 8 hold a stream on its first frame, a learning one and a detecting one (three launch keys).  Batches up to
    step 8, then clips of 3 frames: stream 2 passes detect_after inside a clip call, stream 0 at the start of one.  Every mask, background and packed
    word (528 pixels are no multiple of 64) and the final state of all three streams equal each stream's own single-stream host run."""
    torch = _torch()
    H, W, S, U = 16, 33, 3, 15
    n, Wd = H * W, (H * W + 63) // 64
    p = dict(ml.DEFAULTS, **ml.FAST, detect_after=4)
    join, reset_at = (0, 3, 6), 8
    frames = [sc.frames_of("scripted", H, W, U, 71 + s) for s in range(S)]
    start = list(join)
    lives = {0: host_run(p, frames[0][:reset_at]), 1: host_run(p, frames[1][:U - join[1]]), 2: host_run(p, frames[2][:U - join[2]])}
    again = host_run(p, frames[0][:U - reset_at])  # stream 0 after its reset
    assert any(r[0][5:].any() for r in lives.values())  # detecting frames with foreground
    eng = engine(p, n_streams=S)
    eng.set_geometry(H, W, 3)

    def check(u, s, fg, bg, bits):
        run = again if s == 0 and u >= reset_at else lives[s]
        want, wbg = run[0][u - start[s]], run[1][u - start[s]]
        assert np.array_equal(fg, want), (u, s, int((fg != want).sum()))
        assert np.array_equal(bg, wbg), (u, s)
        assert np.array_equal(bits, words_of(want, Wd)), (u, s)

    u = 0
    while u < U:
        if u == reset_at:
            eng.reset_stream(0)
            start[0] = reset_at
        k = sum(1 for s in range(S) if join[s] <= u)
        if u < 9:
            if u in (6, 8):  # (first frame, past detect_after) differs between all three streams
                assert len({(u - start[s] == 0, u - start[s] >= 4) for s in range(k)}) == 3
            d_frames = torch.from_numpy(np.stack([frames[s][u - start[s]] for s in range(k)])).cuda()
            d_fg = torch.full((k, H, W), 9, dtype=torch.uint8, device="cuda")
            d_bg = torch.full((k, H, W, 3), 9, dtype=torch.uint8, device="cuda")
            d_bits = torch.full((k, Wd), -1, dtype=torch.int64, device="cuda")
            assert eng.process_batch_device(d_frames, d_fg, d_bg, d_bits, first=0, count=k) == BOTH
            torch.cuda.synchronize()
            fg, bg, bits = d_fg.cpu().numpy(), d_bg.cpu().numpy(), d_bits.cpu().numpy().view(np.uint64)
            for s in range(k):
                check(u, s, fg[s], bg[s], bits[s])
            u += 1
        else:
            c = 3
            d_frames = torch.from_numpy(np.stack([np.stack([frames[s][u + j - start[s]] for s in range(S)]) for j in range(c)])).cuda()  # [c][S][H][W][3]
            d_fg = torch.full((c, S, H, W), 9, dtype=torch.uint8, device="cuda")
            d_bg = torch.full((c, S, H, W, 3), 9, dtype=torch.uint8, device="cuda")
            d_bits = torch.full((c, S, Wd), -1, dtype=torch.int64, device="cuda")
            assert eng.process_clip_device(d_frames, c, d_fg, d_bg, d_bits) == [BOTH] * c
            torch.cuda.synchronize()
            fg, bg, bits = d_fg.cpu().numpy(), d_bg.cpu().numpy(), d_bits.cpu().numpy().view(np.uint64)
            for j in range(c):
                for s in range(S):
                    check(u + j, s, fg[j, s], bg[j, s], bits[j, s])
            u += c
    for s, run in ((0, again), (1, lives[1]), (2, lives[2])):
        assert eng.frames_seen(s) == U - start[s]
        same_state(state_of(eng, n, stream=s), run[2], "stream %d" % s)
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
