"""VuMeter (BGS_VUMETER, USTC_BGS type 31) on the MI355X.  Every comparison is exact: masks, backgrounds and
histogram planes equal the reference's own model code (tests/golden/vumeter_ref.npz) and, with the wrapper's filter, the numpy
restatement (tests/vumeter_numpy.py); the dense and the live-bin kernels agree bit for bit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import vumeter_numpy as vn
from test_vumeter_cpu import CASES, GOLDEN, WHOLE_MODEL, golden, masks_of
from tracking_amd import Engine, capi

from gpu_helpers import _torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
BOTH = capi.FG_VALID | capi.BG_VALID


def params(**kw):
    p = capi.default_params(capi.VUMETER)
    for k, v in kw.items():
        setattr(p, "vu_" + k, v)
    return p


def colour_input(case):
    """3-channel frames whose RGB2GRAY image is the fixture's gray input: the committed colour clip, or (v, v, v)."""
    r, p, gray = golden(case)
    if json.loads(str(r["params"]))["input"] == "gray:frames_96x80":
        frames = np.load(os.path.join(GOLDEN, "frames_96x80.npz"))["frames"]
    else:
        frames = np.repeat(gray[..., None], 3, axis=-1)
    assert np.array_equal(vn.gray_rgb(frames), gray)
    return r, p, frames


def run_fixture_case(case):
    r, p, frames = colour_input(case)
    eng = Engine(capi.VUMETER, params=params(enable_filter=0, **p))
    want = masks_of(r)
    for t, f in enumerate(frames):
        fg, bg = eng.process(f)
        assert fg is not None and bg is not None, t  # both valid from the first frame
        assert bg.shape == fg.shape == f.shape[:2]
        assert np.array_equal(fg, want[t]), (case, t, int((fg != want[t]).sum()))
        assert vn.crc(bg) == int(r["bg_crc32"][t]), (case, t)
    assert np.array_equal(bg, r["bg_last"])
    n = frames.shape[1] * frames.shape[2]
    assert int(eng.get_state("count", (1,), np.int64)[0]) == int(r["count"][0])
    assert np.array_equal(eng.get_state("background", (n,), np.uint8), r["bg_last"].reshape(-1))
    if case in WHOLE_MODEL:
        B = r["hist"].shape[0]
        got = eng.get_state("hist", (B, n), np.float32)
        assert np.array_equal(got.view(np.uint32), r["hist"].reshape(B, n).view(np.uint32)), (case, int((got != r["hist"].reshape(B, n)).sum()))
    eng.close()


@pytest.mark.parametrize("case", CASES)
def test_engine_equals_reference_fixture(case):
    run_fixture_case(case)


@pytest.mark.parametrize("sparse", ["0", "2"])
def test_other_kernel_variants_equal_the_fixtures_in_a_fresh_process(sparse):
    """The default is the live-bin kernel with whole-line stores (BGS_VU_SPARSE=1); the dense kernel (0) and the live-bin kernel with
    masked stores (2) run every fixture case again, each in a child process of its own, and report the kernel that ran."""
    code = ("import test_gpu_12_vumeter as t, numpy as np\nfrom tracking_amd import Engine, capi\n"
            "for c in t.CASES:\n    t.run_fixture_case(c)\n"
            "e = Engine(capi.VUMETER); e.enable_kernel_timing(True); e.process(np.zeros((8, 8, 3), np.uint8)); print('ran', e.kernel_timing()[2])\n")
    env = dict(os.environ, BGS_VU_SPARSE=sparse, PYTHONPATH=os.pathsep.join([HERE, os.path.dirname(HERE)]))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, cwd=os.path.dirname(HERE))
    assert r.returncode == 0, r.stdout + r.stderr
    assert ("ran vumeter_kernel<dense>" if sparse == "0" else "ran vumeter_kernel<live,masked>") in r.stdout, r.stdout


def test_default_variant_is_the_live_bin_kernel_and_many_bins_fall_back_to_dense():
    f = np.zeros((8, 8, 3), np.uint8)
    for kw, name in ((dict(), "vumeter_kernel<live>"), (dict(bin_size=7), "vumeter_kernel<dense>"), (dict(bin_size=8), "vumeter_kernel<live>")):
        e = Engine(capi.VUMETER, params=params(**kw))
        e.enable_kernel_timing(True)
        e.process(f)
        assert e.kernel_timing()[2] == name, kw
        e.close()


@pytest.mark.parametrize("T,H,W", [(24, 80, 96), (30, 7, 13), (12, 1, 1), (20, 21, 30)])
def test_filtered_masks_equal_the_restatement(T, H, W):
    """The wrapper with its post-filter (erode 3x3, median 5) on colour frames: frames_96x80, ragged and smaller than a wave, one
    pixel, a width that is no multiple of 4.  Planes after every frame on the small ones."""
    frames = np.load(os.path.join(GOLDEN, "frames_96x80.npz"))["frames"] if (H, W) == (80, 96) else vn.bgr(T, H, W, seed=H * W)
    eng, ref = Engine(capi.VUMETER), vn.VuMeter()
    seen = 0
    for t, f in enumerate(frames):
        fg, bg = eng.process(f)
        wfg, wbg = ref.process(f)
        assert np.array_equal(fg, wfg), (t, int((fg != wfg).sum()))
        assert np.array_equal(bg, wbg), t
        seen += int((wfg != 0).sum())
        if H * W < 1000:
            got = eng.get_state("hist", (32, H * W), np.float32)
            assert np.array_equal(got.view(np.uint32), ref.model.hist.reshape(32, -1).view(np.uint32)), t
    assert seen > 0 or H * W < 100
    eng.close()


def test_streams_of_different_ages_ranges_reset_and_ragged_bits():
    """3 streams started at different frames in one batch and through ranges on two HIP streams, one reset in the middle, a 37 x 53
    geometry (no multiple of 64 nor of 4: the packed words are made from the byte masks), the filter on for even steps and off
    for odd ones (it is live).  Every mask, background, packed word and - at the end - plane equals a per-stream restatement."""
    torch = _torch()
    S, H, W, T = 3, 37, 53, 14
    clips = [vn.bgr(T + 2 * S, H, W, seed=40 + s) for s in range(S)]
    eng = Engine(capi.VUMETER, n_streams=S)
    eng.set_geometry(H, W, 3)
    refs = [vn.VuMeter() for _ in range(S)]
    pos = [0] * S
    for s in range(S):  # stream s has seen 2 s frames: stream 0 is inside its quiet phase when stream 2 has left it
        for _ in range(2 * s):
            eng.process_batch_device(torch.from_numpy(clips[s][pos[s]]).cuda().unsqueeze(0), None, None, None, first=s, count=1)
            refs[s].process(clips[s][pos[s]])
            pos[s] += 1
    Wd = (H * W + 63) // 64
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    seen = 0
    for step in range(T):
        filt = 1 if step % 2 == 0 else 0
        eng.set_params(params(enable_filter=filt))
        d = torch.from_numpy(np.stack([clips[s][pos[s]] for s in range(S)])).cuda()
        d_fg = torch.full((S, H, W), 7, dtype=torch.uint8, device="cuda")
        d_bg = torch.full((S, H, W), 9, dtype=torch.uint8, device="cuda")
        d_bits = torch.zeros((S, Wd), dtype=torch.int64, device="cuda")
        if step == 8:
            eng.reset_stream(1)
            refs[1] = vn.VuMeter()
            assert not eng.get_state("hist", (32, H * W), np.float32, 1).any()
        if step % 3 != 1:
            flags = eng.process_batch_device(d, d_fg, d_bg, d_bits)
            assert flags == BOTH
        else:  # two ranges on two HIP streams, each ordered after the upload
            torch.cuda.current_stream().synchronize()
            eng.process_batch_device(d[:1], d_fg[:1], d_bg[:1], d_bits[:1], hip_stream=s1.cuda_stream, first=0, count=1)
            eng.process_batch_device(d[1:], d_fg[1:], d_bg[1:], d_bits[1:], hip_stream=s2.cuda_stream, first=1, count=2)
            s1.synchronize(), s2.synchronize()
        torch.cuda.synchronize()
        fg, bg, bits = d_fg.cpu().numpy(), d_bg.cpu().numpy(), d_bits.cpu().numpy().view(np.uint64)
        for s in range(S):
            refs[s].enable_filter = filt
            wfg, wbg = refs[s].process(clips[s][pos[s]])
            pos[s] += 1
            assert np.array_equal(fg[s], wfg), (step, s, int((fg[s] != wfg).sum()))
            assert np.array_equal(bg[s], wbg), (step, s)
            packed = np.packbits(wfg.reshape(-1) != 0, bitorder="little")  # tail bits of the last word zero
            wbits = np.zeros(Wd * 8, np.uint8)
            wbits[:len(packed)] = packed
            assert np.array_equal(bits[s], wbits.view(np.uint64)), (step, s)
            assert eng.stream_flags(s) == BOTH and eng.frames_seen(s) == refs[s].model.count
            seen += int((wfg != 0).sum())
    assert seen > 100
    for s in range(S):
        got = eng.get_state("hist", (32, H * W), np.float32, s)
        assert np.array_equal(got.view(np.uint32), refs[s].model.hist.reshape(32, -1).view(np.uint32)), s
        assert int(eng.get_state("count", (1,), np.int64, s)[0]) == refs[s].model.count
    eng.close()


@pytest.mark.parametrize("filt", [0, 1])
def test_packed_only_output_and_more_streams_than_one_table(filt):
    """66 streams of three different ages (more than the 64 per-stream bits of one launch), packed masks only, a pixel count that is
    a multiple of 64 (filter off: words from wave ballots; on: from the filtered byte mask in the engine's own buffer)."""
    torch = _torch()
    S, H, W = 66, 8, 16
    base = vn.bgr(12, H, W, seed=77)
    eng = Engine(capi.VUMETER, n_streams=S, params=params(enable_filter=filt))
    eng.set_geometry(H, W, 3)
    refs = [vn.VuMeter(enable_filter=filt) for _ in range(S)]
    pos = [0] * S
    for s in range(S):
        for _ in range(s % 3 * 3):
            eng.process_batch_device(torch.from_numpy(base[pos[s]]).cuda().unsqueeze(0), None, None, None, first=s, count=1)
            refs[s].process(base[pos[s]])
            pos[s] += 1
    for step in range(3):
        d_bits = torch.zeros((S, H * W // 64), dtype=torch.int64, device="cuda")
        d_bg = torch.zeros((S, H, W), dtype=torch.uint8, device="cuda")
        eng.process_batch_device(torch.from_numpy(np.stack([base[pos[s]] for s in range(S)])).cuda(), None, d_bg, d_bits)
        torch.cuda.synchronize()
        bits, bg = d_bits.cpu().numpy().view(np.uint64), d_bg.cpu().numpy()
        for s in range(S):
            wfg, wbg = refs[s].process(base[pos[s]])
            pos[s] += 1
            assert np.array_equal(bits[s], np.packbits(wfg.reshape(-1) != 0, bitorder="little").view(np.uint64)), (step, s)
            assert np.array_equal(bg[s], wbg), (step, s)
    eng.close()


def test_device_path_clip_and_submit_equal_host_path():
    torch = _torch()
    frames = vn.bgr(10, 20, 32, seed=5)
    host, dev, lane, clip = (Engine(capi.VUMETER) for _ in range(4))
    dev.set_geometry(20, 32, 3)
    outs = []
    for f in frames:
        fg, bg = host.process(f)
        outs.append((fg, bg))
        d_fg = torch.zeros((1, 20, 32), dtype=torch.uint8, device="cuda")
        d_bg = torch.zeros((1, 20, 32), dtype=torch.uint8, device="cuda")
        assert dev.process_batch_device(torch.from_numpy(f).cuda().unsqueeze(0), d_fg, d_bg, None) == BOTH
        torch.cuda.synchronize()
        assert np.array_equal(d_fg.cpu().numpy()[0], fg) and np.array_equal(d_bg.cpu().numpy()[0], bg)
        lfg, lbg = np.zeros((20, 32), np.uint8), np.zeros((20, 32), np.uint8)
        lane.submit(np.ascontiguousarray(f), lfg, lbg)
        assert lane.wait() == BOTH
        assert np.array_equal(lfg, fg) and np.array_equal(lbg, bg)
    clip.set_geometry(20, 32, 3)  # a clip runs one launch per frame
    c_fg = torch.zeros((10, 1, 20, 32), dtype=torch.uint8, device="cuda")
    c_bg = torch.zeros((10, 1, 20, 32), dtype=torch.uint8, device="cuda")
    assert clip.process_clip_device(torch.from_numpy(frames).cuda().unsqueeze(1), 10, c_fg, c_bg) == [BOTH] * 10
    torch.cuda.synchronize()
    for t, (fg, bg) in enumerate(outs):
        assert np.array_equal(c_fg.cpu().numpy()[t, 0], fg) and np.array_equal(c_bg.cpu().numpy()[t, 0], bg), t
    for e in (host, dev, lane, clip):
        e.close()


def test_set_params_after_the_first_frame_keeps_the_model_parameters_and_takes_the_filter():
    frames = vn.bgr(16, 18, 22, seed=9)
    kw = dict(bin_size=16, alpha=0.9, threshold=0.3)
    eng, ref = Engine(capi.VUMETER, params=params(**kw)), vn.VuMeter(**kw)
    for t, f in enumerate(frames):
        if t == 6:  # SetAlpha / SetBinSize / SetThreshold ran on the first frame only; enableFilter is re-read every frame
            eng.set_params(params(bin_size=4, alpha=0.5, threshold=0.9, enable_filter=0))
            ref.enable_filter = 0
        fg, bg = eng.process(f)
        wfg, wbg = ref.process(f)
        assert np.array_equal(fg, wfg) and np.array_equal(bg, wbg), t
    got = eng.get_state("hist", (16, 18 * 22), np.float32)
    assert np.array_equal(got.view(np.uint32), ref.model.hist.reshape(16, -1).view(np.uint32))
    eng.close()


def test_gray_frames_and_groups_are_refused():
    import ctypes as C
    eng = Engine(capi.VUMETER)
    with pytest.raises(capi.BgsError) as ei:
        eng.process(np.zeros((12, 16), np.uint8))
    assert ei.value.code == capi.ERR_UNSUPPORTED and "VuMeter" in str(ei.value)
    eng.close()
    algos = (C.c_int * 2)(capi.FRAME_DIFF, capi.VUMETER)
    g = C.c_void_p()
    assert capi.lib().bgs_group_create(algos, None, 2, 0, 1, C.byref(g)) == capi.ERR_UNSUPPORTED and b"VuMeter" in capi.lib().bgs_last_error()


def frame_1080(t, base, noise):
    f = base + np.roll(noise, (t * 7) % 97, axis=1)
    y, x = (t * 90) % 700, (t * 170) % 1400
    f[y:y + 300, x:x + 400] = (t * 40) % 256
    return np.clip(f, 0, 255).astype(np.uint8)


def test_two_1080p_streams_equal_restatement_on_a_pixel_sample():
    """The model is pointwise before the filter, so the filter is off and the restatement runs on the sampled pixels only."""
    torch = _torch()
    S, H, W, T = 2, 1080, 1920, 8
    rng = np.random.default_rng(31)
    bases = [rng.integers(30, 220, (H, W, 3)).astype(np.int16) for _ in range(S)]
    noises = [rng.integers(-6, 7, (H, W, 3)).astype(np.int16) for _ in range(S)]
    edges = np.concatenate([np.arange(0, 130), W + np.arange(0, 96), H * W - 1 - np.arange(130)])
    sample = np.unique(np.concatenate([rng.integers(0, H * W, 65536), edges]))[:65536]
    eng = Engine(capi.VUMETER, n_streams=S, params=params(enable_filter=0))
    eng.set_geometry(H, W, 3)
    refs, bgs = [vn.Model() for _ in range(S)], [None] * S
    seen_fg = 0
    for t in range(T):
        frames = np.stack([frame_1080(t, bases[s], noises[s]) for s in range(S)])
        d_fg = torch.zeros((S, H, W), dtype=torch.uint8, device="cuda")
        d_bg = torch.zeros((S, H, W), dtype=torch.uint8, device="cuda")
        d_bits = torch.zeros((S, H * W // 64), dtype=torch.int64, device="cuda")
        assert eng.process_batch_device(torch.from_numpy(frames).cuda(), d_fg, d_bg, d_bits) == BOTH
        torch.cuda.synchronize()
        fg, bg, bits = d_fg.cpu().numpy().reshape(S, -1), d_bg.cpu().numpy().reshape(S, -1), d_bits.cpu().numpy().view(np.uint64)
        for s in range(S):
            gray = vn.gray_rgb(frames[s]).reshape(-1)[sample][None]
            if bgs[s] is None:
                bgs[s] = gray.copy()
            wfg = refs[s].update(gray, bgs[s])[0]
            assert np.array_equal(fg[s][sample], wfg), (t, s, int((fg[s][sample] != wfg).sum()))
            assert np.array_equal(bg[s][sample], bgs[s][0]), (t, s)
            assert np.array_equal(bits[s], np.packbits(fg[s] != 0, bitorder="little").view(np.uint64)), (t, s)
            seen_fg += int((wfg != 0).sum())
    assert seen_fg > 500
    for s in range(S):
        got = eng.get_state("hist", (32, H * W), np.float32, s)[:, sample]
        assert np.array_equal(got.view(np.uint32), refs[s].hist.reshape(32, -1).view(np.uint32)), s
    eng.close()


def test_demo_ustc_type_31_and_frame_processor_equal_the_restatement(tmp_path):
    """The host C++ layer: USTC_BGS(31) (tracker path) and FrameProcessor with enableVuMeter, non-default parameters through
    ./config/VuMeter.xml, against the restatement (filter on) and the fixture (filter off, case thr_edge)."""
    from test_gpu_01_host_cpp import HOST, DEMO, write_fp_config
    subprocess.run(["make", "-s", "-C", HOST], check=True)
    r, p, clip = colour_input("thr_edge")
    n, rows, cols = clip.shape[:3]
    raw = str(tmp_path / "vu.raw")
    clip.tofile(raw)
    for filt in (0, 1):
        if filt:
            ref = vn.VuMeter(enable_filter=1, **p)
            want = np.stack([ref.process(f)[0] for f in clip])
        else:
            want = masks_of(r)
        xml = "<enableFilter>%d</enableFilter>\n<binSize>8</binSize>\n<alpha>%r</alpha>\n<threshold>%r</threshold>\n" % (filt, p["alpha"], p["threshold"])
        for mode in ("ustc", "fp"):
            wd = tmp_path / ("vu_%s_%d" % (mode, filt))
            (wd / "config").mkdir(parents=True)
            (wd / "config" / "VuMeter.xml").write_text('<?xml version="1.0"?>\n<opencv_storage>\n%s</opencv_storage>\n' % xml)
            if mode == "ustc":
                args = [DEMO, raw, str(rows), str(cols), str(n), str(wd / "out"), "31", "shapes"]
                out = wd / "out.ustc.raw"
            else:
                write_fp_config(str(wd / "config"), set())
                with open(str(wd / "config" / "FrameProcessor.xml")) as f:
                    text = f.read().replace("</opencv_storage>", "<enableVuMeter>1</enableVuMeter>\n</opencv_storage>")
                with open(str(wd / "config" / "FrameProcessor.xml"), "w") as f:
                    f.write(text)
                args = [DEMO, raw, str(rows), str(cols), str(n), str(wd / "out")]
                out = wd / "out.VuMeter.raw"
            res = subprocess.run(args, cwd=str(wd), capture_output=True, text=True)
            assert res.returncode == 0, res.stdout + res.stderr
            got = np.fromfile(str(out), np.uint8).reshape(n, rows, cols)
            assert np.array_equal(got, want), (mode, filt, int((got != want).sum()))
            if mode == "ustc":  # mask and background model are 8UC1: the background is the gray image the model keeps
                shapes = [l for l in res.stdout.split("\n") if l.startswith("frame ")]
                assert shapes == ["frame %d mask %dx%dx1 background %dx%dx1" % (t, rows, cols, rows, cols) for t in range(n)], shapes[:3]
            saved = (wd / "config" / "VuMeter.xml").read_text()
            assert "<showOutput>1</showOutput>" in saved and "<enableFilter>%d</enableFilter>" % filt in saved and "<binSize>8</binSize>" in saved
