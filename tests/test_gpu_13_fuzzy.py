"""FuzzySugenoIntegral / FuzzyChoquetIntegral (BGS_FUZZY_SUGENO / BGS_FUZZY_CHOQUET, USTC_BGS types 21 and 22) on the MI355X.  Every
output is float32 IEEE arithmetic without libm, so every comparison is exact: masks, background bytes, the float
background and the integral plane equal the reference's own FuzzyUtils / PixelUtils (tests/golden/fuzzy_ref.npz) and, on frames the
fixture does not hold, the numpy restatement (tests/fuzzy_numpy.py), whose permutation prefix is computed independently."""
import os
import subprocess

import numpy as np
import pytest

import fuzzy_numpy as fz
from test_fuzzy_cpu import CASES, check_against_fixture, golden, masks_of
from tracking_amd import Engine, capi

from gpu_helpers import _torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
BOTH = capi.FG_VALID | capi.BG_VALID
ALGO = {fz.SUGENO: capi.FUZZY_SUGENO, fz.CHOQUET: capi.FUZZY_CHOQUET}
FIELDS = dict(ftl="frames_to_learn", alphaLearn="alpha_learn", alphaUpdate="alpha_update", option="option", smooth="smooth", threshold="threshold")


def set_params(eng, p):
    eng.set_fuzzy_params(**{FIELDS[k]: v for k, v in p.items()})


def state_of(eng, H, W, stream=0):
    return eng.get_state("background", (H, W, 3), np.float32, stream), eng.get_state("integral", (H, W), np.float32, stream)


def same(a, b):
    """Bit for bit, NaNs by position."""
    nan = np.isnan(b)
    return np.array_equal(np.isnan(a), nan) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan])


@pytest.mark.parametrize("case", CASES)
def test_engine_equals_reference_fixture(case):
    r, _, frames = golden(case)
    H, W = frames.shape[1:3]
    eng = Engine(ALGO[int(r["kind"])])

    def step(f, p):
        set_params(eng, p)
        return eng.process(f)

    check_against_fixture(case, step, lambda: state_of(eng, H, W))
    assert int(eng.get_state("count", (1,), np.int64)[0]) == len(frames)
    eng.close()


def seeded(T, H, W, seed):
    """A noisy background with a moving box: both mask values, ties (equal bytes) and different orderings of the three similarities."""
    rng = np.random.default_rng(seed)
    base = rng.integers(20, 236, (H, W, 3))
    out = []
    for t in range(T):
        f = base + rng.integers(-12, 13, (H, W, 3)) * (rng.random((H, W, 1)) < 0.7)
        y, x = (3 * t) % max(H - 1, 1), (5 * t) % max(W - 1, 1)
        f[y:y + max(H // 3, 1), x:x + max(W // 3, 1)] = rng.integers(0, 256, 3)
        out.append(np.clip(f, 0, 255).astype(np.uint8))
    return np.stack(out)


@pytest.mark.parametrize("kind", [fz.CHOQUET, fz.SUGENO])
@pytest.mark.parametrize("H,W", [(45, 67), (67, 45), (2, 2), (3, 3), (9, 2), (2, 9)])
def test_engine_equals_restatement_on_seeded_frames(kind, H, W):
    """67x45 (W x H): odd, landscape, less than two scan blocks; 45x67: portrait; the smallest frames; one column / row pair of 2."""
    frames = seeded(7, H, W, seed=H * 100 + W)
    kw = dict(ftl=2, option=2 if H < 10 else 1 + (H > W))
    eng, ref = Engine(ALGO[kind]), fz.Fuzzy(kind, **kw)
    set_params(eng, kw)
    for t, f in enumerate(frames):
        fg, bg = eng.process(f)
        wfg, wbg = ref.process(f)
        assert (fg is None) == (wfg is None) == (t <= 2), t
        if wfg is not None:
            assert np.array_equal(fg, wfg), (t, int((fg != wfg).sum()))
            assert np.array_equal(bg, wbg), t
            gb, gi = state_of(eng, H, W)
            assert same(gi, ref.integral), (t, int((gi != ref.integral).sum()))
            assert same(gb, ref.bg), t
            mm = eng.get_state("minmax", (2,), np.float32)
            assert mm[0] == min(np.float32(255), ref.integral.min()) and mm[1] == max(np.float32(0), ref.integral.max())
    eng.close()


def test_three_qvga_streams_with_different_content_do_not_leak_into_each_other():
    """One detecting frame of 320x240 (75 scan blocks per stream) for 3 streams in one batch: sigma and min / max are per stream."""
    torch = _torch()
    S, H, W = 3, 240, 320
    clips = [seeded(3, H, W, seed=900 + s) for s in range(S)]
    eng = Engine(capi.FUZZY_CHOQUET, n_streams=S)
    eng.set_geometry(H, W, 3)
    eng.set_fuzzy_params(frames_to_learn=1)
    refs = [fz.Fuzzy(fz.CHOQUET, ftl=1) for _ in range(S)]
    for t in range(3):
        d_fg = torch.full((S, H, W), 7, dtype=torch.uint8, device="cuda")
        d_bg = torch.full((S, H, W, 3), 9, dtype=torch.uint8, device="cuda")
        flags = eng.process_batch_device(torch.from_numpy(np.stack([c[t] for c in clips])).cuda(), d_fg, d_bg, None)
        torch.cuda.synchronize()
        assert flags == (BOTH if t == 2 else 0)
        for s in range(S):
            wfg, wbg = refs[s].process(clips[s][t])
            if t < 2:
                assert wfg is None and (d_fg[s] == 7).all() and (d_bg[s] == 9).all()  # outputs untouched while learning
                continue
            fg, bg = d_fg[s].cpu().numpy(), d_bg[s].cpu().numpy()
            assert np.array_equal(fg, wfg), (s, int((fg != wfg).sum()))
            assert np.array_equal(bg, wbg), s
            gb, gi = state_of(eng, H, W, s)
            assert same(gi, refs[s].integral) and same(gb, refs[s].bg), s
    assert len({refs[s].integral.min() for s in range(S)}) == S  # the streams' minima differ, so a shared one would show
    eng.close()


def test_streams_of_different_ages_share_a_launch_reset_and_live_parameters():
    """Stream 1 starts three frames late, so for a while one stream learns and the other detects in the same batch call; stream 0 is
    reset in the middle; the threshold, alphaUpdate and smooth change between frames; raising frames_to_learn sends both back to
    learning.  37 x 53 is no multiple of 64: the packed words come from the byte masks."""
    torch = _torch()
    S, H, W, T = 2, 37, 53, 16
    clips = [seeded(T + 3, H, W, seed=60 + s) for s in range(S)]
    eng = Engine(capi.FUZZY_SUGENO, n_streams=S)
    eng.set_geometry(H, W, 3)
    kw = dict(ftl=2)
    set_params(eng, kw)
    refs = [fz.Fuzzy(fz.SUGENO, **kw) for _ in range(S)]
    pos = [0, 0]
    for _ in range(3):
        eng.process_batch_device(torch.from_numpy(clips[0][pos[0]]).cuda().unsqueeze(0), None, None, None, first=0, count=1)
        refs[0].process(clips[0][pos[0]])
        pos[0] += 1
    Wd = (H * W + 63) // 64
    mixed = fg_seen = 0
    for step in range(T):
        if step == 5:
            kw = dict(threshold=0.8, alphaUpdate=0.05, smooth=0)
        if step == 8:
            eng.reset_stream(0)
            refs[0] = fz.Fuzzy(fz.SUGENO, **refs[0].p)
            assert eng.frames_seen(0) == 0 and int(eng.get_state("count", (1,), np.int64, 0)[0]) == 0
        if step == 12:
            kw = dict(ftl=100)
        if step == 14:
            kw = dict(ftl=1, smooth=1)
        set_params(eng, kw)
        d = torch.from_numpy(np.stack([clips[s][pos[s]] for s in range(S)])).cuda()
        d_fg = torch.full((S, H, W), 7, dtype=torch.uint8, device="cuda")
        d_bg = torch.full((S, H, W, 3), 9, dtype=torch.uint8, device="cuda")
        d_bits = torch.zeros((S, Wd), dtype=torch.int64, device="cuda")
        flags = eng.process_batch_device(d, d_fg, d_bg, d_bits)
        torch.cuda.synchronize()
        want = []
        for s in range(S):
            want.append(refs[s].process(clips[s][pos[s]], **kw))
            pos[s] += 1
        valid = [w[0] is not None for w in want]
        mixed += valid[0] != valid[1]
        assert flags == (BOTH if all(valid) else 0), step
        bits = d_bits.cpu().numpy().view(np.uint64)
        for s in range(S):
            assert eng.stream_flags(s) == (BOTH if valid[s] else 0), (step, s)
            assert int(eng.get_state("count", (1,), np.int64, s)[0]) == refs[s].frame_number
            if not valid[s]:
                assert (d_fg[s] == 7).all() and (d_bg[s] == 9).all(), (step, s)
                continue
            fg = d_fg[s].cpu().numpy()
            assert np.array_equal(fg, want[s][0]), (step, s, int((fg != want[s][0]).sum()))
            assert np.array_equal(d_bg[s].cpu().numpy(), want[s][1]), (step, s)
            packed = np.packbits(fg.reshape(-1) != 0, bitorder="little")
            wbits = np.zeros(Wd * 8, np.uint8)
            wbits[:len(packed)] = packed
            assert np.array_equal(bits[s], wbits.view(np.uint64)), (step, s)
            fg_seen += int((fg != 0).sum())
        for s in range(S):
            assert same(eng.get_state("background", (H, W, 3), np.float32, s), refs[s].bg), (step, s)
    assert mixed >= 3 and fg_seen > 100
    q = eng.get_fuzzy_params()
    assert (q.frames_to_learn, q.smooth, q.threshold, q.alpha_update) == (1, 1, 0.8, 0.05)
    eng.close()


def test_refusals_on_the_engine_and_groups():
    import ctypes as C
    for algo, name in ((capi.FUZZY_SUGENO, "FuzzySugenoIntegral"), (capi.FUZZY_CHOQUET, "FuzzyChoquetIntegral")):
        eng = Engine(algo)
        for frame in (np.zeros((12, 16), np.uint8), np.zeros((1, 16, 3), np.uint8), np.zeros((12, 1, 3), np.uint8)):
            with pytest.raises(capi.BgsError) as ei:
                eng.process(frame)
            assert ei.value.code == capi.ERR_UNSUPPORTED and name in str(ei.value)
        for kw in (dict(color_space=2), dict(color_space=3), dict(color_space=4), dict(option=0)):
            with pytest.raises(capi.BgsError) as ei:
                eng.set_fuzzy_params(**kw)
            assert ei.value.code == capi.ERR_UNSUPPORTED and name in str(ei.value)
        assert eng.process(np.zeros((2, 2, 3), np.uint8)) == (None, None)  # still usable, with the values it had
        with pytest.raises(capi.BgsError) as ei:  # the geometry is set now: a refusal stays a refusal and leaves the values alone
            eng.set_fuzzy_params(option=3)
        assert ei.value.code == capi.ERR_UNSUPPORTED and name in str(ei.value) and eng.get_fuzzy_params().option == 2
        eng.close()
    with pytest.raises(capi.BgsError):
        Engine(capi.VUMETER).set_fuzzy_params(option=1)
    algos = (C.c_int * 2)(capi.FRAME_DIFF, capi.FUZZY_CHOQUET)
    g = C.c_void_p()
    assert capi.lib().bgs_group_create(algos, None, 2, 0, 1, C.byref(g)) == capi.ERR_UNSUPPORTED and b"fuzzy" in capi.lib().bgs_last_error()


def test_device_path_clip_and_submit_equal_host_path():
    torch = _torch()
    H, W = 20, 32
    frames = seeded(8, H, W, seed=5)
    host, dev, lane, clip = (Engine(capi.FUZZY_CHOQUET) for _ in range(4))
    for e in (host, dev, lane, clip):
        e.set_geometry(H, W, 3)
        e.set_fuzzy_params(frames_to_learn=3)
    outs = []
    for t, f in enumerate(frames):
        fg, bg = host.process(f)
        outs.append((fg, bg))
        want = BOTH if t > 3 else 0
        assert (fg is not None) == (t > 3)
        d_fg = torch.zeros((1, H, W), dtype=torch.uint8, device="cuda")
        d_bg = torch.zeros((1, H, W, 3), dtype=torch.uint8, device="cuda")
        assert dev.process_batch_device(torch.from_numpy(f).cuda().unsqueeze(0), d_fg, d_bg, None) == want
        torch.cuda.synchronize()
        lfg, lbg = np.zeros((H, W), np.uint8), np.zeros((H, W, 3), np.uint8)
        lane.submit(np.ascontiguousarray(f), lfg, lbg)
        assert lane.wait() == want
        if want:
            assert np.array_equal(d_fg.cpu().numpy()[0], fg) and np.array_equal(d_bg.cpu().numpy()[0], bg)
            assert np.array_equal(lfg, fg) and np.array_equal(lbg, bg)
    c_fg = torch.zeros((8, 1, H, W), dtype=torch.uint8, device="cuda")
    c_bg = torch.zeros((8, 1, H, W, 3), dtype=torch.uint8, device="cuda")
    assert clip.process_clip_device(torch.from_numpy(frames).cuda().unsqueeze(1), 8, c_fg, c_bg) == [0] * 4 + [BOTH] * 4
    torch.cuda.synchronize()
    for t, (fg, bg) in enumerate(outs):
        if fg is not None:
            assert np.array_equal(c_fg.cpu().numpy()[t, 0], fg) and np.array_equal(c_bg.cpu().numpy()[t, 0], bg), t
    for e in (host, dev, lane, clip):
        e.close()


@pytest.mark.parametrize("case,ustc", [("sugeno_opt1", 21), ("choquet_opt1", 22)])
def test_demo_ustc_types_21_22_and_frame_processor_equal_the_fixture(tmp_path, case, ustc):
    """The host C++ layer: USTC_BGS(21 / 22) (tracker path) and FrameProcessor with enableFuzzy*Integral, the case's non-default
    parameters through ./config/Fuzzy*Integral.xml; untouched outputs (learning frames) are dumped as 7s by the demo."""
    from test_gpu_01_host_cpp import HOST, DEMO, write_fp_config
    subprocess.run(["make", "-s", "-C", HOST], check=True)
    r, plist, clip = golden(case)
    n, rows, cols = clip.shape[:3]
    name = "FuzzySugenoIntegral" if ustc == 21 else "FuzzyChoquetIntegral"
    want = np.full((n, rows, cols), 7, np.uint8)
    want[r["valid"] != 0] = masks_of(r, cols)
    for t in range(1, n):  # GetMask() / img_fsi keep the last mask; there is none before the first detecting frame
        if not r["valid"][t] and r["valid"][:t].any():
            want[t] = want[t - 1]
    raw = str(tmp_path / "fz.raw")
    clip.tofile(raw)
    p = plist[0]
    xml = ("<showOutput>0</showOutput>\n<framesToLearn>%d</framesToLearn>\n<alphaLearn>%r</alphaLearn>\n<alphaUpdate>%r</alphaUpdate>\n<colorSpace>1</colorSpace>\n"
           "<option>%d</option>\n<smooth>%d</smooth>\n<threshold>%r</threshold>\n" % (p["ftl"], p["alphaLearn"], p["alphaUpdate"], p["option"], p["smooth"], p["threshold"]))
    for mode in ("ustc", "fp"):
        wd = tmp_path / mode
        (wd / "config").mkdir(parents=True)
        (wd / "config" / (name + ".xml")).write_text('<?xml version="1.0"?>\n<opencv_storage>\n%s</opencv_storage>\n' % xml)
        if mode == "ustc":
            args = [DEMO, raw, str(rows), str(cols), str(n), str(wd / "out"), str(ustc)]
            out = wd / "out.ustc.raw"
        else:
            write_fp_config(str(wd / "config"), set())
            path = str(wd / "config" / "FrameProcessor.xml")
            text = open(path).read().replace("</opencv_storage>", "<enable%s>1</enable%s>\n</opencv_storage>" % (name, name))
            open(path, "w").write(text)
            args = [DEMO, raw, str(rows), str(cols), str(n), str(wd / "out")]
            out = wd / ("out.%s.raw" % name)
        res = subprocess.run(args, cwd=str(wd), capture_output=True, text=True)
        assert res.returncode == 0, res.stdout + res.stderr
        got = np.fromfile(str(out), np.uint8).reshape(n, rows, cols)
        assert np.array_equal(got, want), (mode, int((got != want).sum()))
        saved = (wd / "config" / (name + ".xml")).read_text()
        assert saved.index("<showOutput>") < saved.index("<framesToLearn>") < saved.index("<option>") < saved.index("<threshold>")
