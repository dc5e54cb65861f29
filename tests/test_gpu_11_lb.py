"""The five package_bgs/lb/ models (BGS_LB_*, USTC_BGS types 25-29) on the MI355X.  Parity contract: the three
classes without exp() equal the reference's own code (tests/golden/lb_ref_*.npz) and the numpy restatement (tests/lb_numpy.py) bit
for bit - masks, background bytes, every model plane; the two fuzzy classes equal them exactly in masks and background bytes and
within lb_numpy.FUZZY_PLANE_TOL in the model planes (the device's exp() and glibc's may differ in the last bit)."""
import subprocess

import numpy as np
import pytest

import lb_numpy as ln
from test_lb_cpu import ALGO, CASES, CLASSES, FUZZY, WHOLE_MODEL, golden, masks_of
from tracking_amd import Engine, capi

from gpu_helpers import _torch

pytestmark = pytest.mark.gpu


def params_of(cls, **kw):
    p = capi.default_params(getattr(capi, ALGO[cls]))
    for k, v in kw.items():
        setattr(p, "lb_" + k, v)
    return p


def engine(cls, n_streams=1, **kw):
    return Engine(getattr(capi, ALGO[cls]), params=params_of(cls, **kw), n_streams=n_streams)


def planes_of(eng, cls, n, stream=0):
    f8 = np.float64
    if cls in (25, 26):
        return {"mu": eng.get_state("mu", (n, 3), f8, stream), "var": eng.get_state("var", (n, 3), f8, stream)}
    if cls == 27:
        return {"w": eng.get_state("w", (n, 3), f8, stream), "mu": eng.get_state("mu", (n, 3, 3), f8, stream), "var": eng.get_state("var", (n, 3, 3), f8, stream),
                "sortkey": eng.get_state("sortkey", (n, 3), f8, stream), "k": eng.get_state("k", (n,), np.int32, stream)}
    return {"som": eng.get_state("som", (n, 3, 3, 3), f8, stream), "bg": eng.get_state("bg", (n, 3), np.uint8, stream),
            "count": eng.get_state("count", (1,), np.int64, stream)}


def assert_planes(cls, got, want, where, idx=None):
    """Exact for 25 / 27 / 28 and for the byte and integer planes; the fuzzy classes' doubles within FUZZY_PLANE_TOL."""
    for name, w in want.items():
        g = got[name]
        if idx is not None and name != "count":
            g = g[idx]
        w = np.asarray(w).reshape(g.shape)
        tol = ln.FUZZY_PLANE_TOL[cls].get(name) if cls in FUZZY else None
        if tol is None:
            assert np.array_equal(g, w), (where, name, int((g != w).sum()))
        else:
            d = float(np.abs(g - w).max())
            assert d <= tol, (where, name, d, tol)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("cls", CLASSES)
def test_engine_equals_reference_fixture(cls, case):
    r, p, change, frames = golden(cls, case)
    eng = engine(cls, **p)
    want = masks_of(r)
    for t, f in enumerate(frames):
        if change and t == change[0]:
            eng.set_params(params_of(cls, **dict(p, **change[1])))
        fg, bg = eng.process(f)
        assert fg is not None and bg is not None, t  # both valid from the first frame
        assert np.array_equal(fg, want[t]), (cls, case, t, int((fg != want[t]).sum()))
        assert ln.crc(bg) == int(r["bg_crc32"][t]), (cls, case, t)
    assert np.array_equal(bg, r["bg_last"])
    if case in WHOLE_MODEL:
        n = frames.shape[1] * frames.shape[2]
        want_planes = {k: r[k] for k in planes_of(eng, cls, n) if k in r}
        assert len(want_planes) >= 2
        assert_planes(cls, planes_of(eng, cls, n), want_planes, (cls, case))
    eng.close()


@pytest.mark.parametrize("cls", CLASSES)
def test_every_plane_follows_the_restatement_after_every_frame(cls):
    """A small tie-heavy clip with a fast learning rate: exact zeros at the d*d guards, variances on their clamps, ties in the BMU
    search and in the first-hit match."""
    kw = {25: dict(learning_rate=200, noise_variance=40), 26: dict(learning_rate=200, noise_variance=40), 27: dict(learning_rate=180, noise_variance=40),
          28: dict(learning_rate=220, training_steps=7, sensitivity=120), 29: dict(learning_rate=220, training_steps=7, sensitivity=120)}[cls]
    frames = ln.tie_clip(36, 13, 11, seed=60 + cls)
    eng, ref = engine(cls, **kw), ln.LB(cls, **kw)
    n = 13 * 11
    for t, f in enumerate(frames):
        fg, bg = eng.process(f)
        wfg, wbg = ref.process(f)
        assert np.array_equal(fg, wfg) and np.array_equal(bg, wbg), (cls, t)
        assert_planes(cls, planes_of(eng, cls, n), ref.planes(), (cls, t))
    eng.close()


@pytest.mark.parametrize("cls", CLASSES)
def test_streams_of_different_ages_ranges_reset_and_ragged_bits(cls):
    """4 streams started at different frames in one batch and through ranges on two HIP streams, a reset in the middle (the stream
    re-runs Init with the constructor's noise and restarts m_K), a 37 x 53 geometry (not a multiple of 64 nor of 4: the packed
    words straddle streams).  Every mask, background, packed word and - at the end - plane equals a per-stream restatement."""
    torch = _torch()
    S, H, W, T = 4, 37, 53, 14
    kw = dict(training_steps=6) if cls in (28, 29) else {}
    clips = [ln.noisy_clip(T + S, H, W, seed=70 + 10 * cls + s, box=0.15) for s in range(S)]
    eng = engine(cls, n_streams=S, **kw)
    eng.set_geometry(H, W, 3)
    refs = [ln.LB(cls, **kw) for _ in range(S)]
    pos = [0] * S

    def feed(s):
        want = refs[s].process(clips[s][pos[s]])
        pos[s] += 1
        return want

    for s in range(S):  # stream s has seen s frames: the SOMs' training counters differ inside one launch
        for _ in range(s):
            d = torch.from_numpy(clips[s][pos[s]]).cuda().unsqueeze(0)
            eng.process_batch_device(d, None, None, None, first=s, count=1)
            feed(s)
    Wd = (H * W + 63) // 64
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for step in range(T):
        frames = np.stack([clips[s][pos[s]] for s in range(S)])
        d = torch.from_numpy(frames).cuda()
        d_fg = torch.full((S, H, W), 7, dtype=torch.uint8, device="cuda")
        d_bg = torch.full((S, H, W, 3), 9, dtype=torch.uint8, device="cuda")
        d_bits = torch.zeros((S, Wd), dtype=torch.int64, device="cuda")
        if step == 8:
            eng.reset_stream(2)
            refs[2] = ln.LB(cls, **kw)
        if step % 2 == 0:
            eng.process_batch_device(d, d_fg, d_bg, d_bits)
        else:  # two ranges on two HIP streams, each ordered after the upload
            torch.cuda.current_stream().synchronize()
            eng.process_batch_device(d[:1], d_fg[:1], d_bg[:1], d_bits[:1], hip_stream=s1.cuda_stream, first=0, count=1)
            eng.process_batch_device(d[1:], d_fg[1:], d_bg[1:], d_bits[1:], hip_stream=s2.cuda_stream, first=1, count=3)
            s1.synchronize(), s2.synchronize()
        torch.cuda.synchronize()
        fg, bg, bits = d_fg.cpu().numpy(), d_bg.cpu().numpy(), d_bits.cpu().numpy().view(np.uint64)
        for s in range(S):
            wfg, wbg = feed(s)
            assert np.array_equal(fg[s], wfg), (cls, step, s, int((fg[s] != wfg).sum()))
            assert np.array_equal(bg[s], wbg), (cls, step, s)
            packed = np.packbits(wfg.reshape(-1) != 0, bitorder="little")  # tail bits of the last word zero
            wbits = np.zeros(Wd * 8, np.uint8)
            wbits[:len(packed)] = packed
            assert np.array_equal(bits[s], wbits.view(np.uint64)), (cls, step, s)
            assert eng.stream_flags(s) == capi.FG_VALID | capi.BG_VALID
            assert eng.frames_seen(s) == refs[s].fn
    for s in range(S):
        assert_planes(cls, planes_of(eng, cls, H * W, s), refs[s].planes(), (cls, "end", s))
    eng.close()


@pytest.mark.parametrize("cls", CLASSES)
def test_more_streams_than_one_launch_has_table_entries(cls):
    """20 streams whose ages all differ (more than the 16 per-stream table entries of one SOM launch), packed masks only, a pixel
    count that is a multiple of 64 (words from wave ballots)."""
    torch = _torch()
    S, H, W = 20, 16, 24
    kw = dict(training_steps=30) if cls in (28, 29) else {}
    clips = [ln.noisy_clip(S + 3, H, W, seed=900 + s) for s in range(S)]
    eng = engine(cls, n_streams=S, **kw)
    eng.set_geometry(H, W, 3)
    refs = [ln.LB(cls, **kw) for _ in range(S)]
    pos = [0] * S
    for s in range(S):
        for _ in range(s):
            eng.process_batch_device(torch.from_numpy(clips[s][pos[s]]).cuda().unsqueeze(0), None, None, None, first=s, count=1)
            refs[s].process(clips[s][pos[s]])
            pos[s] += 1
    for step in range(3):
        frames = np.stack([clips[s][pos[s]] for s in range(S)])
        d_bits = torch.zeros((S, H * W // 64), dtype=torch.int64, device="cuda")
        d_bg = torch.zeros((S, H, W, 3), dtype=torch.uint8, device="cuda")
        eng.process_batch_device(torch.from_numpy(frames).cuda(), None, d_bg, d_bits)
        torch.cuda.synchronize()
        bits, bg = d_bits.cpu().numpy().view(np.uint64), d_bg.cpu().numpy()
        for s in range(S):
            wfg, wbg = refs[s].process(clips[s][pos[s]])
            pos[s] += 1
            assert np.array_equal(bits[s], np.packbits(wfg.reshape(-1) != 0, bitorder="little").view(np.uint64)), (cls, step, s)
            assert np.array_equal(bg[s], wbg), (cls, step, s)
    eng.close()


@pytest.mark.parametrize("cls", CLASSES)
def test_live_parameter_change_equals_the_restatement(cls):
    frames = ln.noisy_clip(24, 18, 22, seed=300 + cls)
    a = {25: dict(sensitivity=90), 26: dict(sensitivity=90), 27: dict(sensitivity=90), 28: dict(training_steps=15), 29: dict(training_steps=15)}[cls]
    b = {25: dict(sensitivity=30, noise_variance=220, learning_rate=100), 26: dict(sensitivity=30, bg_threshold=50, noise_variance=220, learning_rate=100),
         27: dict(sensitivity=30, bg_threshold=230, noise_variance=220, learning_rate=100),
         28: dict(sensitivity=30, training_sensitivity=80, learning_rate=100, training_learning_rate=150, training_steps=4),
         29: dict(sensitivity=30, training_sensitivity=80, learning_rate=100, training_learning_rate=150, training_steps=4)}[cls]
    eng, ref = engine(cls, **a), ln.LB(cls, **a)
    for t, f in enumerate(frames):
        if t == 9:
            eng.set_params(params_of(cls, **dict(a, **b)))
            ref.set(**b)
        fg, bg = eng.process(f)
        wfg, wbg = ref.process(f)
        assert np.array_equal(fg, wfg) and np.array_equal(bg, wbg), (cls, t)
    assert_planes(cls, planes_of(eng, cls, 18 * 22), ref.planes(), (cls, "end"))
    bad = params_of(cls, **dict(a, sensitivity=300))
    with pytest.raises(capi.BgsError) as ei:
        eng.set_params(bad)
    assert ei.value.code == capi.ERR_UNSUPPORTED and ln.NAMES[cls] in str(ei.value)
    eng.close()


def frame_1080(t, base, noise):
    f = base + np.roll(noise, (t * 7) % 97, axis=1)
    y, x = (t * 90) % 700, (t * 170) % 1400
    f[y:y + 300, x:x + 400] = (t * 40) % 256
    return np.clip(f, 0, 255).astype(np.uint8)


@pytest.mark.parametrize("cls", CLASSES)
def test_two_1080p_streams_equal_restatement_on_a_pixel_sample(cls):
    torch = _torch()
    S, H, W, T = 2, 1080, 1920, 6
    rng = np.random.default_rng(5 + cls)
    bases = [rng.integers(30, 220, (H, W, 3)).astype(np.int16) for _ in range(S)]
    noises = [rng.integers(-6, 7, (H, W, 3)).astype(np.int16) for _ in range(S)]
    edges = np.concatenate([np.arange(0, 130), W + np.arange(0, 96), H * W - 1 - np.arange(130)])
    sample = np.unique(np.concatenate([rng.integers(0, H * W, 4000), edges]))
    kw = dict(training_steps=3) if cls in (28, 29) else {}
    eng = engine(cls, n_streams=S, **kw)
    eng.set_geometry(H, W, 3)
    refs = [ln.LB(cls, pixels=sample, **kw) for _ in range(S)]
    Wd = H * W // 64
    seen_fg = 0
    for t in range(T):
        frames = np.stack([frame_1080(t, bases[s], noises[s]) for s in range(S)])
        d = torch.from_numpy(frames).cuda()
        d_fg = torch.zeros((S, H, W), dtype=torch.uint8, device="cuda")
        d_bg = torch.zeros((S, H, W, 3), dtype=torch.uint8, device="cuda")
        d_bits = torch.zeros((S, Wd), dtype=torch.int64, device="cuda")
        flags = eng.process_batch_device(d, d_fg, d_bg, d_bits)
        torch.cuda.synchronize()
        assert flags == capi.FG_VALID | capi.BG_VALID
        fg, bg, bits = d_fg.cpu().numpy().reshape(S, -1), d_bg.cpu().numpy().reshape(S, -1, 3), d_bits.cpu().numpy().view(np.uint64)
        for s in range(S):
            wfg, wbg = refs[s].process(frames[s])
            wfg, wbg = wfg.reshape(-1), wbg.reshape(-1, 3)
            assert np.array_equal(fg[s][sample], wfg[sample]), (cls, t, s, int((fg[s][sample] != wfg[sample]).sum()))
            assert np.array_equal(bg[s][sample], wbg[sample]), (cls, t, s)
            assert np.array_equal(bits[s], np.packbits(fg[s] != 0, bitorder="little").view(np.uint64)), (cls, t, s)
            seen_fg += int((wfg[sample] != 0).sum())
    assert seen_fg > 500
    for s in range(S):
        assert_planes(cls, planes_of(eng, cls, H * W, s), refs[s].planes(), (cls, "end", s), idx=sample)
    eng.close()


@pytest.mark.parametrize("cls", CLASSES)
def test_device_path_equals_host_path_submit_wait_and_gray_is_refused(cls):
    torch = _torch()
    frames = ln.noisy_clip(8, 20, 32, seed=500 + cls)
    host, dev, lane = engine(cls), engine(cls), engine(cls)
    dev.set_geometry(20, 32, 3)
    for f in frames:
        fg, bg = host.process(f)
        d_fg = torch.zeros((1, 20, 32), dtype=torch.uint8, device="cuda")
        d_bg = torch.zeros((1, 20, 32, 3), dtype=torch.uint8, device="cuda")
        dev.process_batch_device(torch.from_numpy(f).cuda().unsqueeze(0), d_fg, d_bg, None)
        torch.cuda.synchronize()
        assert np.array_equal(d_fg.cpu().numpy()[0], fg) and np.array_equal(d_bg.cpu().numpy()[0], bg)
        lfg, lbg = np.zeros((20, 32), np.uint8), np.zeros((20, 32, 3), np.uint8)
        lane.submit(np.ascontiguousarray(f), lfg, lbg)
        assert lane.wait() == capi.FG_VALID | capi.BG_VALID
        assert np.array_equal(lfg, fg) and np.array_equal(lbg, bg)
    for e in (host, dev, lane):
        e.close()
    gray = engine(cls)
    with pytest.raises(capi.BgsError) as ei:
        gray.process(frames[0][:, :, 0].copy())
    assert ei.value.code == capi.ERR_UNSUPPORTED and ln.NAMES[cls] in str(ei.value)
    gray.close()


def test_demo_ustc_types_25_29_and_frame_processor_equal_fixture(tmp_path):
    """The host C++ layer: USTC_BGS(25..29) (tracker path) and FrameProcessor with the five enableLB* flags, non-default parameters
    through ./config/<Class>.xml, against the reference's own masks (case "params")."""
    from test_gpu_01_host_cpp import HOST, DEMO, write_fp_config
    subprocess.run(["make", "-s", "-C", HOST], check=True)
    xml_key = {"sensitivity": "sensitivity", "bg_threshold": "bgThreshold", "learning_rate": "learningRate", "noise_variance": "noiseVariance",
               "training_sensitivity": "trainingSensitivity", "training_learning_rate": "trainingLearningRate", "training_steps": "trainingSteps"}
    for cls in CLASSES:
        name = ln.NAMES[cls]
        r, p, change, clip = golden(cls, "params")
        want = masks_of(r)
        xml = "".join("<%s>%d</%s>\n" % (xml_key[k], v, xml_key[k]) for k, v in p.items())
        raw = str(tmp_path / ("%s.raw" % name))
        clip.tofile(raw)
        n, rows, cols = clip.shape[:3]
        for mode in ("ustc", "fp"):
            wd = tmp_path / ("%s_%s" % (name, mode))
            (wd / "config").mkdir(parents=True)
            (wd / "config" / ("%s.xml" % name)).write_text('<?xml version="1.0"?>\n<opencv_storage>\n%s</opencv_storage>\n' % xml)
            if mode == "ustc":
                args = [DEMO, raw, str(rows), str(cols), str(n), str(wd / "out"), str(cls), "shapes"]
                out = wd / "out.ustc.raw"
            else:
                write_fp_config(str(wd / "config"), set())
                with open(str(wd / "config" / "FrameProcessor.xml")) as f:
                    text = f.read().replace("</opencv_storage>", "<enable%s>1</enable%s>\n</opencv_storage>" % (name, name))
                with open(str(wd / "config" / "FrameProcessor.xml"), "w") as f:
                    f.write(text)
                args = [DEMO, raw, str(rows), str(cols), str(n), str(wd / "out")]
                out = wd / ("out.%s.raw" % name)
            res = subprocess.run(args, cwd=str(wd), capture_output=True, text=True)
            assert res.returncode == 0, res.stdout + res.stderr
            got = np.fromfile(str(out), np.uint8).reshape(n, rows, cols)
            assert np.array_equal(got, want), (name, mode, int((got != want).sum()))
            if mode == "ustc":  # the wrappers hand out cv::Mat(m_pBGModel->GetFG()): an 8UC3 mask (the file above holds its first channel)
                shapes = [l for l in res.stdout.split("\n") if l.startswith("frame ")]
                assert len(shapes) == n and all(" mask %dx%dx3 " % (rows, cols) in l for l in shapes), shapes[:3]
            saved = (wd / "config" / ("%s.xml" % name)).read_text()
            assert "<showOutput>1</showOutput>" in saved and "<sensitivity>%d</sensitivity>" % p["sensitivity"] in saved


@pytest.mark.parametrize("cls", [25, 26])
def test_two_pixels_per_lane_variant_gives_identical_results(cls, monkeypatch):
    """BGS_LB_PX=2 (the double2 form of the Gaussian kernels) against the restatement: an even pixel count takes
    it, an odd one falls back to one pixel per lane; packed words from the pair-wise shuffle."""
    torch = _torch()
    monkeypatch.setenv("BGS_LB_PX", "2")
    for H, W in ((16, 24), (13, 11)):
        S = 3
        clips = [ln.noisy_clip(6, H, W, seed=700 + s) for s in range(S)]
        eng = engine(cls, n_streams=S)
        eng.set_geometry(H, W, 3)
        refs = [ln.LB(cls) for _ in range(S)]
        Wd = (H * W + 63) // 64
        for t in range(6):
            d_fg = torch.zeros((S, H, W), dtype=torch.uint8, device="cuda")
            d_bg = torch.zeros((S, H, W, 3), dtype=torch.uint8, device="cuda")
            d_bits = torch.zeros((S, Wd), dtype=torch.int64, device="cuda")
            eng.process_batch_device(torch.from_numpy(np.stack([c[t] for c in clips])).cuda(), d_fg, d_bg, d_bits)
            torch.cuda.synchronize()
            fg, bg, bits = d_fg.cpu().numpy(), d_bg.cpu().numpy(), d_bits.cpu().numpy().view(np.uint64)
            for s in range(S):
                wfg, wbg = refs[s].process(clips[s][t])
                assert np.array_equal(fg[s], wfg) and np.array_equal(bg[s], wbg), (cls, H, W, t, s)
                packed = np.packbits(wfg.reshape(-1) != 0, bitorder="little")
                wbits = np.zeros(Wd * 8, np.uint8)
                wbits[:len(packed)] = packed
                assert np.array_equal(bits[s], wbits.view(np.uint64)), (cls, H, W, t, s)
        for s in range(S):
            assert_planes(cls, planes_of(eng, cls, H * W, s), refs[s].planes(), (cls, H, W, s))
        eng.close()
