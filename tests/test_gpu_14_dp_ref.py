"""The five package_bgs/dp models on the GPU against the outputs of the reference's own code (tests/golden/dp_ref_*.npz, read through
tests/dp_ref.py; nothing here needs the reference tree): the per-frame host path on every case, the batch path with streams that
share a state tile, the fused clip path of the two GMMs for every K, both forms of the median kernel on the wrapping thresholds,
parameters frozen at the first frame, and the host classes with a wrapping threshold in their XML."""
import os
import subprocess

import numpy as np
import pytest

import dp_ref
from gpu_helpers import STATE_TOL, _torch, max_err
from tracking_amd import Engine, capi

pytestmark = pytest.mark.gpu

ALL = [(cls, case) for cls in dp_ref.CLASSES for case in dp_ref.cases(cls)]
OBSERVED = {}  # class -> largest float-plane difference against the fixtures seen in this run (printed; DESIGN.md §4 quotes it)


def check_planes(cls, eng, want, p, n, stream=0, where=""):
    """Float planes within STATE_TOL of the fixture's bits, mode counts and median bytes equal."""
    for name, w in want.items():
        shape, dt = dp_ref.plane_shape(cls, name, p, n)
        got = eng.get_state(name, shape, dt, stream=stream)
        if dt == np.uint8:
            assert np.array_equal(got, w), "%s %s %s" % (cls, where, name)
        else:
            assert np.array_equal(np.isnan(got), np.isnan(w)), "%s %s %s: NaN pattern" % (cls, where, name)
            err = max_err(got, w)
            OBSERVED[cls] = max(OBSERVED.get(cls, 0.0), err)
            print("%s %s %s: max |delta| against the reference's bits %g" % (cls, where, name, err))
            assert err <= STATE_TOL, "%s %s %s: max |delta| %g" % (cls, where, name, err)


def oracle_planes(cls, r):
    """Planes of a case too large to be stored: from the CPU oracle, which test_dp_cpu.py pins to the reference bit for bit."""
    return dp_ref.oracle_run(cls, r["params"], r["frames"], dp_ref.CLASSES[cls][2])[1]


@pytest.mark.parametrize("cls,case", ALL, ids=["%s-%s" % cc for cc in ALL])
def test_host_path_matches_reference_fixture(cls, case):
    r = dp_ref.load(cls)[case]
    frames, p = r["frames"], r["params"]
    eng = Engine(dp_ref.CLASSES[cls][1], params=dp_ref.engine_params(cls, p))
    for t, f in enumerate(frames):
        fg, bg = eng.process(f, want_bg=False)
        assert bg is None and np.array_equal(fg, r["masks"][t]), "frame %d: %d mask pixels differ" % (t, int((fg != r["masks"][t]).sum()))
    check_planes(cls, eng, r["planes"], p, frames.shape[1] * frames.shape[2], where=case)
    eng.close()


@pytest.mark.parametrize("cls", list(dp_ref.CLASSES))
def test_batch_path_streams_share_a_state_tile(cls):
    """S = 3 streams of 37 x 53 = 1 961 pixels: the tiled state puts pixels of two streams into tiles 7 and 15, and the launch covers
    5 883 pixels (not a multiple of 4, 64 or 256).  Stream k enters the clip k frames late (fixture cases ragged, ragged_o1, ragged_o2)."""
    torch = _torch()
    cases = dp_ref.load(cls)
    rs = [cases[c] for c in ("ragged", "ragged_o1", "ragged_o2")]
    S, (T, H, W) = 3, rs[0]["masks"].shape
    n, words = H * W, (H * W + 63) // 64
    assert n % 256 and (n - 1) // 256 == n // 256  # the last pixel of a stream and the first of the next lie in one tile
    p = rs[0]["params"]
    eng = Engine(dp_ref.CLASSES[cls][1], params=dp_ref.engine_params(cls, p), n_streams=S)
    eng.set_geometry(H, W, 3)
    for t in range(T):
        d_frames = torch.from_numpy(np.stack([r["frames"][t] for r in rs])).cuda()
        d_fg = torch.full((S, H, W), 9, dtype=torch.uint8, device="cuda")
        d_bits = torch.full((S, words), -1, dtype=torch.int64, device="cuda")
        flags = eng.process_batch_device(d_frames, d_fg, None, d_bits)
        torch.cuda.synchronize()
        assert flags == capi.FG_VALID
        fg = d_fg.cpu().numpy()
        bits = np.unpackbits(d_bits.cpu().numpy().view(np.uint8).reshape(S, -1), axis=1, bitorder="little")
        for s in range(S):
            want = rs[s]["masks"][t]
            assert np.array_equal(fg[s], want), (t, s, int((fg[s] != want).sum()))
            assert np.array_equal(bits[s, :n], (want != 0).ravel()), (t, s)
            assert not bits[s, n:].any(), "tail bits of the last word must be zero"
    for s in range(S):
        check_planes(cls, eng, oracle_planes(cls, rs[s]), p, n, stream=s, where="stream %d" % s)
    eng.close()


@pytest.mark.parametrize("case", ["modes_k1", "modes_k2", "modes", "modes_k4", "modes_k5", "modes_ties"])
@pytest.mark.parametrize("cls", ["ziv", "grim"])
def test_fused_clip_path_matches_reference_fixture(cls, case):
    """process_clip_device with 4 frames per call: dp_gmm_kernel<K, GRIMSON> keeps the model in registers over the four frames.
    Every K the kernel is built for, against the reference's masks and its whole model."""
    torch = _torch()
    r = dp_ref.load(cls)[case]
    frames, p = r["frames"], r["params"]
    T, H, W = r["masks"].shape
    NC = 4
    assert T % NC == 0
    eng = Engine(dp_ref.CLASSES[cls][1], params=dp_ref.engine_params(cls, p))
    eng.set_geometry(H, W, 3)
    for t0 in range(0, T, NC):
        d_frames = torch.from_numpy(np.array(frames[t0:t0 + NC, None])).cuda()  # [NC][1][H][W][3]
        d_fg = torch.full((NC, 1, H, W), 9, dtype=torch.uint8, device="cuda")
        flags = eng.process_clip_device(d_frames, NC, d_fg, None, None)
        torch.cuda.synchronize()
        assert all(f == capi.FG_VALID for f in flags)
        fg = d_fg.cpu().numpy()[:, 0]
        assert np.array_equal(fg, r["masks"][t0:t0 + NC]), (t0, int((fg != r["masks"][t0:t0 + NC]).sum()))
    assert eng.frames_seen(0) == T
    check_planes(cls, eng, r["planes"], p, H * W, where=case + " clip")
    eng.close()


@pytest.mark.parametrize("cls", ["ziv", "grim"])
def test_write_back_gives_the_same_bytes_frame_by_frame_fused_and_unfused(cls):
    """alpha06_k4 (40 frames of 8 x 14, K = 4, alpha 0.6) three ways: one process_batch_device call per frame, process_clip_device in
    calls of 8 frames (one launch each, the model in registers), and the same calls with BGS_OPT_CLIP_FUSE 0.  Every mask and the
    model equal the fixture's, and the raw bytes of `modes` and `nmodes` are the same in all three, slots above the count included:
    the write-back rule (a field is stored if its bits changed, or if its slot was not loaded and was in use after ANY frame of the
    launch).  ziv: the counts read after every frame must show, in every run of 8, a pixel whose count peaks above both its value at
    the run's start and at its end - a slot that comes into use and is pruned again inside one launch, which only that rule writes.
    grim never shrinks a count at an alpha in [0, 1): there the K = 4 sort and the stale `significants` above the count are pinned."""
    torch = _torch()
    r = dp_ref.load(cls)["alpha06_k4"]
    p = r["params"]
    T, H, W = r["masks"].shape
    n, NC = H * W, 8
    assert (T, H, W, p["gaussians"]) == (40, 8, 14, 4)
    shape, _ = dp_ref.plane_shape(cls, "modes", p, n)
    d_all = torch.from_numpy(np.array(r["frames"][:, None])).cuda()  # [T][1][H][W][3]

    def engine():
        eng = Engine(dp_ref.CLASSES[cls][1], params=dp_ref.engine_params(cls, p))
        eng.set_geometry(H, W, 3)
        eng.enable_kernel_timing(True)
        return eng

    def finish(eng, launches, where):
        _, nl, name = eng.kernel_timing()
        assert (nl, name) == (launches, "dp_gmm_kernel"), (where, nl, name)
        check_planes(cls, eng, r["planes"], p, n, where="alpha06_k4 " + where)
        model = eng.get_state("modes", shape, np.float32).tobytes(), eng.get_state("nmodes", (n,), np.uint8).tobytes()
        eng.close()
        return model

    eng = engine()
    counts = np.zeros((T + 1, n), np.int64)  # counts[t + 1]: after frame t
    for t in range(T):
        d_fg = torch.full((1, H, W), 9, dtype=torch.uint8, device="cuda")
        assert eng.process_batch_device(d_all[t], d_fg, None, None) == capi.FG_VALID
        torch.cuda.synchronize()
        assert np.array_equal(d_fg.cpu().numpy()[0], r["masks"][t]), (t, "frame by frame")
        counts[t + 1] = eng.get_state("nmodes", (n,), np.uint8)
    models = {"frame by frame": finish(eng, T, "frame by frame")}
    if cls == "ziv":
        for t0 in range(0, T, NC):
            peak = counts[t0 + 1:t0 + NC + 1].max(axis=0)
            came_and_went = int(((peak > counts[t0]) & (peak > counts[t0 + NC])).sum())
            print("ziv frames %d-%d: %d of %d pixels bring a slot into use and lose it again" % (t0, t0 + NC - 1, came_and_went, n))
            assert came_and_went >= 1, t0
    for fuse, launches in ((1, T // NC), (0, T)):
        eng = engine()
        eng.set_option(capi.OPT_CLIP_FUSE, fuse)
        for t0 in range(0, T, NC):
            d_fg = torch.full((NC, 1, H, W), 9, dtype=torch.uint8, device="cuda")
            flags = eng.process_clip_device(d_all[t0:t0 + NC], NC, d_fg, None, None)
            torch.cuda.synchronize()
            assert flags == [capi.FG_VALID] * NC
            fg = d_fg.cpu().numpy()[:, 0]
            assert np.array_equal(fg, r["masks"][t0:t0 + NC]), (fuse, t0, int((fg != r["masks"][t0:t0 + NC]).sum()))
        assert eng.frames_seen(0) == T
        models["fuse %d" % fuse] = finish(eng, launches, "fuse %d" % fuse)
    for where, model in models.items():
        assert model == models["frame by frame"], "%s: modes / nmodes bytes differ from the frame-by-frame run" % where


@pytest.mark.parametrize("case,form", [("tile", 4), ("tile_t130", 4), ("tile_t300", 4), ("ragged", 1), ("ragged_t130", 1), ("ragged_t300", 1)])
def test_both_median_kernel_forms_on_device_buffers(case, form):
    """dp_median_kernel<4> (pixel count a multiple of 4, torch's aligned buffers) and dp_median_kernel<1> through the device path,
    byte and packed masks, on default and wrapping thresholds (130 -> high 4, 300 -> low 44)."""
    torch = _torch()
    r = dp_ref.load("median")[case]
    T, H, W = r["masks"].shape
    n, words = H * W, (H * W + 63) // 64
    assert (n % 4 == 0) == (form == 4)
    eng = Engine(capi.DP_ADAPTIVE_MEDIAN, params=dp_ref.engine_params("median", r["params"]))
    eng.set_geometry(H, W, 3)
    for t in range(T):
        d_frames = torch.from_numpy(np.array(r["frames"][t][None])).cuda()
        d_fg = torch.full((1, H, W), 9, dtype=torch.uint8, device="cuda")
        d_bits = torch.full((1, words), -1, dtype=torch.int64, device="cuda")
        eng.process_batch_device(d_frames, d_fg, None, d_bits)
        torch.cuda.synchronize()
        assert np.array_equal(d_fg.cpu().numpy()[0], r["masks"][t]), t
        bits = np.unpackbits(d_bits.cpu().numpy().view(np.uint8).ravel(), bitorder="little")
        assert np.array_equal(bits[:n], (r["masks"][t] != 0).ravel()) and not bits[n:].any(), t
    want = r["planes"] or oracle_planes("median", r)
    check_planes("median", eng, want, r["params"], n, where=case)
    eng.close()


@pytest.mark.parametrize("cls", list(dp_ref.CLASSES))
def test_parameters_are_frozen_at_the_first_frame(cls):
    """The wrappers hand their members to the model inside `if(firstTime)` only: set_params with another threshold, alpha, number
    of gaussians and sampling rate at frame 5 changes nothing - masks and model still equal the reference's for the first values."""
    r = dp_ref.load(cls)["tile"]
    frames, p = r["frames"], r["params"]
    eng = Engine(dp_ref.CLASSES[cls][1], params=dp_ref.engine_params(cls, p))
    for t, f in enumerate(frames):
        if t == 5:
            q = dp_ref.engine_params(cls, p)
            q.dp_threshold, q.dp_alpha, q.dp_gaussians, q.dp_sampling_rate, q.learning_frames = 130.0, 0.4, 5, 1, 0
            eng.set_params(q)
        fg, _ = eng.process(f, want_bg=False)
        assert np.array_equal(fg, r["masks"][t]), t
    check_planes(cls, eng, r["planes"], p, frames.shape[1] * frames.shape[2], where="frozen")
    eng.close()


def test_host_classes_take_the_wrapping_thresholds_from_their_xml(tmp_path):
    """DPAdaptiveMedianBGS with <threshold>130</threshold> gives the reference's mask (high threshold 4, not 260), DPMeanBGS with
    -1 an empty one, through the C++ host classes and their XML files."""
    from test_gpu_01_host_cpp import CLASSES, DEMO, HOST, run_demo, write_fp_config
    subprocess.run(["make", "-s", "-C", HOST], check=True)
    r = dp_ref.load("median")["tile_t130"]
    frames = r["frames"]
    write_fp_config(str(tmp_path / "config"), ["DPAdaptiveMedianBGS", "DPMeanBGS"])
    assert {"DPAdaptiveMedianBGS", "DPMeanBGS"} <= set(CLASSES)
    (tmp_path / "config" / "DPAdaptiveMedianBGS.xml").write_text(
        '<?xml version="1.0"?>\n<opencv_storage>\n<threshold>130</threshold>\n<samplingRate>7</samplingRate>\n<learningFrames>30</learningFrames>\n<showOutput>0</showOutput>\n</opencv_storage>\n')
    (tmp_path / "config" / "DPMeanBGS.xml").write_text(
        '<?xml version="1.0"?>\n<opencv_storage>\n<threshold>-1</threshold>\n<alpha>0.5</alpha>\n<learningFrames>30</learningFrames>\n<showOutput>0</showOutput>\n</opencv_storage>\n')
    res = run_demo(DEMO, str(tmp_path), frames)
    assert res.returncode == 0, res.stdout + res.stderr
    T, H, W = r["masks"].shape
    got = np.fromfile(str(tmp_path / "out.DPAdaptiveMedianBGS.raw"), np.uint8).reshape(T, H, W)
    assert np.array_equal(got, r["masks"]) and r["masks"][1:].mean() > 100
    assert not np.fromfile(str(tmp_path / "out.DPMeanBGS.raw"), np.uint8).any()
    assert os.path.exists(tmp_path / "config" / "DPMeanBGS.xml")


def test_print_observed_plane_differences():
    """Runs last in this file: the largest float-plane difference per class that the tests above met (pytest -s shows it)."""
    for cls, err in sorted(OBSERVED.items()):
        print("observed max |delta| against the reference fixtures, %s: %g" % (cls, err))
        assert err <= STATE_TOL
