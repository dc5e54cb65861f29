"""SJN_MultiCueBGS as a class on the GPU: streams of one bgs_multicue handle at different ages, one of them restarted
while the others go on; disjoint ranges of a handle on two HIP streams; the refusals; the call that takes a frame in host memory; and
the C++ class through FrameProcessor::enableMultiCueBGS.  Every comparison is byte for byte, against the reference-built fixture
tests/golden/multicue_box_ref.npz or against the numpy restatement tests/multicue_box_numpy.Step that the fixture pins; nothing here
needs the reference tree."""
import ctypes as C
import functools
import subprocess

import numpy as np
import pytest

import multicue_box_numpy as mb
import multicue_numpy as mc
import multicue_scenes as sc
from gpu_helpers import _torch
from tracking_amd import capi
from tracking_amd.engine import MultiCueModel

pytestmark = pytest.mark.gpu
FIX = mb.load()


def params_of(p):
    return capi.multicue_default_params(**{k: p[k] for k in mc.FIELDS})


def geometry(rh, rw, **kw):
    return dict(mc.DEFAULTS, reduced_width=rw, reduced_height=rh, **kw)


def code(call, *a, **kw):
    with pytest.raises(capi.BgsError) as e:
        call(*a, **kw)
    return e.value.code


def snapshot(model):
    return {k: np.array(v, copy=True) for k, v in model.state().items() if k in mc.PLANES}


@functools.lru_cache(maxsize=None)
def restated(rh, rw, rows, cols, seed, stops):
    """The restatement on frames_of("scripted", rows, cols, 30, train, seed) with the FAST periods: (frames, images [30][rows][cols], {frames
    seen: state planes} for every entry of `stops`).  Made once per scene and left unchanged."""
    p = geometry(rh, rw, **mc.FAST)
    train = p["training_period"] + 1
    frames = sc.frames_of("scripted", rows, cols, 30, train, seed)
    step = mb.Step(p)
    images, states = [], {}
    for t, f in enumerate(frames):
        images.append(step.process(f))
        if t + 1 in stops:
            states[t + 1] = snapshot(step.m)
    assert step.box_overflow == 0 and step.m.overflow == 0
    images = np.array(images)
    for a in (frames, images):
        a.setflags(write=False)
    return frames, images, states


def same_state(m, stream, want, where):
    for k in mc.PLANES:
        assert m.state(k, stream).tobytes() == np.ascontiguousarray(want[k]).tobytes(), (where, k)


def test_late_joins_and_a_reset_of_one_stream():
    """Three cameras on one handle.  Stream k joins 2k steps late, so the first steps hold streams that train beside streams that have not
    started and, from step 5, beside one that detects.  Stream 1 is reset at step 12, while it detects, and fed its clip again: steps
    12-16 hold a training stream between two detecting ones, three runs in one call.  Every image is that stream's own restatement
    run, a reset stream shows a new handle's planes, and at the end every plane of every stream is the restatement's at that stream's
    frame count."""
    torch = _torch()
    p = geometry(30, 40, **mc.FAST)
    train, S, steps, reset_at = p["training_period"] + 1, 3, 30, 12
    runs = [restated(30, 40, 60, 85, 171 + k, (steps, steps - reset_at, steps - 4)) for k in range(S)]
    for frames, want, _ in runs:
        assert not want[:train].any() and all(im.any() for im in want[train:])  # foreground in every detecting frame that is compared
    with MultiCueModel(params_of(p), n_streams=S) as m, MultiCueModel(params_of(p), n_streams=1) as new:
        fed = [0] * S  # frames of its clip each stream has seen in its present life
        for u in range(steps):
            if u == reset_at:
                assert fed[1] == reset_at - 2 > train and m.frames_seen(1) == p["training_period"] + 2  # it detects
                m.reset_stream(1)
                fed[1] = 0
                assert m.frames_seen(1) == 0 and m.frames_seen(0) == m.frames_seen(2) == p["training_period"] + 2
                for k in mc.PLANES:
                    assert m.state(k, 1).tobytes() == new.state(k, 0).tobytes(), ("after the reset", k)
            joined = sum(1 for k in range(S) if 2 * k <= u)
            if reset_at <= u < reset_at + train:
                assert joined == S and fed[0] >= train and fed[1] < train and fed[2] >= train  # detecting, training, detecting
            batch = np.stack([runs[k][0][fed[k]] for k in range(joined)])
            got = m.process(torch.from_numpy(batch).cuda(), first=0, count=joined).cpu().numpy()
            for k in range(joined):
                assert np.array_equal(got[k], runs[k][1][fed[k]]), ("step", u, "stream", k, "frame", fed[k])
                fed[k] += 1
        assert fed == [steps, steps - reset_at, steps - 4]
        for k in range(S):
            same_state(m, k, runs[k][2][fed[k]], ("stream", k))
            assert m.frames_seen(k) == p["training_period"] + 2
        assert m.state("overflow")[0] == 0 and m.state("box_overflow")[0] == 0


def test_disjoint_ranges_on_two_hip_streams():
    """Four cameras at the fixture's 37 x 53 frames and 12 x 16 reduced size: streams [0, 2) on one HIP stream and [2, 4) on another, for
    all 30 frames with nothing between them but the end.  Stream 0 is the fixture's clip and gives the reference's images; the others
    give the restatement's; and all four equal the same frames run as one call."""
    torch = _torch()
    f = FIX["step"]["step_12x16"]
    p, train, S = f["params"], f["train"], 4
    assert p == geometry(12, 16, **mc.FAST) and f["frames"].shape == (30, 37, 53, 3)
    seeded = [restated(12, 16, 37, 53, seed, ()) for seed in (181, 182, 183)]
    want = [f["images"]] + [r[1] for r in seeded]
    # at this size the reference's own images hold empty detecting frames (13 of its 25), so not every compared frame can be non-zero:
    # 12, 13, 15 and 11 of the 25 are
    assert [sum(bool(im.any()) for im in w[train:]) for w in want] == [12, 13, 15, 11] and not any(w[:train].any() for w in want)
    clips = torch.from_numpy(np.stack([f["frames"]] + [r[0] for r in seeded], axis=1)).cuda()  # [T][S]: a range of one frame is contiguous
    side = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    with MultiCueModel(params_of(p), n_streams=S) as two, MultiCueModel(params_of(p), n_streams=S) as one:
        halves = []
        for t in range(len(clips)):
            halves.append([two.process(clips[t, 2 * h:2 * h + 2], first=2 * h, count=2, hip_stream=side[h].cuda_stream) for h in range(2)])
        torch.cuda.synchronize()
        got = np.array([np.concatenate([h.cpu().numpy() for h in pair]) for pair in halves])  # [T][S][rows][cols]
        whole = np.array([one.process(clips[t]).cpu().numpy() for t in range(len(clips))])
        for s in range(S):
            assert np.array_equal(got[:, s], whole[:, s]), ("ranges against one call, stream", s)
            assert np.array_equal(got[:, s], want[s]), ("stream", s, np.nonzero((got[:, s] != want[s]).any((1, 2)))[0][:8])
            for k in mc.PLANES:
                assert two.state(k, s).tobytes() == one.state(k, s).tobytes(), (s, k)
        assert [mc.crc(im) for im in got[:, 0]] == list(f["image_crc"])
        assert two.state("overflow")[0] == 0 and two.state("box_overflow")[0] == 0


def test_refusals():
    torch = _torch()
    p = geometry(12, 16, **mc.FAST)

    def zeros(*shape):
        return torch.zeros(shape, dtype=torch.uint8, device="cuda")

    with MultiCueModel(params_of(p), n_streams=2) as m:
        f2, f1 = zeros(2, 37, 53, 3), zeros(1, 37, 53, 3)
        m.train(f2)  # in lock step the piecewise calls work
        m.process(f1, first=1, count=1)
        assert (m.frames_seen(0), m.frames_seen(1)) == (1, 2)
        # the ages differ: the piecewise calls are refused and name the call that is not
        lm, um = zeros(2, 12, 16), torch.ones((2, 12, 16), dtype=torch.uint8, device="cuda")
        for call, args in ((m.train, (f2,)), (m.landmark, (f2,)), (m.update, (um,)), (m.boxes, (lm, f2))):
            assert code(call, *args) == capi.ERR_STATE, call
            assert b"bgs_multicue_process_range_device" in capi.lib().bgs_last_error(), call
        # ranges and stream numbers outside the handle
        for first, count in ((1, 2), (2, 1), (-1, 1), (0, 3), (0, 0), (1, -1)):
            assert code(m.process, zeros(max(count, 0), 37, 53, 3), first=first, count=count) == capi.ERR_INVALID, (first, count)
        for s in (-1, 2):
            assert code(m.reset_stream, s) == capi.ERR_INVALID and code(m.state, "count", s) == capi.ERR_INVALID
            assert code(m.process_host, np.zeros((37, 53, 3), np.uint8), stream=s) == capi.ERR_INVALID
        # another frame size, on the device and from the host
        assert code(m.process, zeros(1, 36, 53, 3), first=0, count=1) == capi.ERR_GEOMETRY
        assert code(m.process, zeros(2, 37, 54, 3)) == capi.ERR_GEOMETRY
        assert code(m.process_host, np.zeros((36, 53, 3), np.uint8)) == capi.ERR_GEOMETRY
        # row pitches below the row size, and a channel count that is neither 1 nor 3
        frame, out = np.zeros((37, 53, 3), np.uint8), np.zeros((37, 53, 3), np.uint8)
        host = capi.lib().bgs_multicue_process
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        assert host(m._h, 0, ptr(frame), 37, 53, 53 * 3 - 1, ptr(out), 53 * 3, 3) == capi.ERR_INVALID
        assert host(m._h, 0, ptr(frame), 37, 53, 53 * 3, ptr(out), 53 * 3 - 1, 3) == capi.ERR_INVALID
        assert host(m._h, 0, ptr(frame), 37, 53, 53 * 3, ptr(out), 52, 1) == capi.ERR_INVALID
        assert host(m._h, 0, ptr(frame), 37, 53, 53 * 3, ptr(out), 53 * 3, 2) == capi.ERR_INVALID
        # nothing above moved a stream, and the range call still takes both
        assert (m.frames_seen(0), m.frames_seen(1)) == (1, 2)
        assert not m.process(f2).any() and (m.frames_seen(0), m.frames_seen(1)) == (2, 3)
        assert host(m._h, 0, ptr(frame), 37, 53, 53 * 3, ptr(out), 53 * 3, 3) == capi.OK and m.frames_seen(0) == 3
        # with every stream restarted the ages agree again
        m.reset_stream(0), m.reset_stream(1)
        m.train(f2)
        assert (m.frames_seen(0), m.frames_seen(1)) == (1, 1)


@pytest.mark.parametrize("channels", [1, 3])
def test_host_path_on_the_fixture_clip(channels):
    """bgs_multicue_process on the reference's 12 x 16 clip, the frames taken from an array with padded rows: the one-channel images are
    the fixture's, and the three channels of a 3-channel output are equal."""
    f = FIX["step"]["step_12x16"]
    T, rows, cols = f["frames"].shape[:3]
    assert f["images"][f["train"]:].any() and not f["images"][:f["train"]].any()
    padded = np.full((T, rows, cols + 5, 3), 0xa5, np.uint8)
    padded[:, :, :cols] = f["frames"]
    clip = padded[:, :, :cols]
    assert clip.strides[1] == (cols + 5) * 3 and not clip[0].flags.c_contiguous
    with MultiCueModel(params_of(f["params"])) as m:
        got = np.array([m.process_host(clip[t], channels=channels) for t in range(T)])
        assert m.frames_seen(0) == f["params"]["training_period"] + 2 and m.state("overflow")[0] == 0 and m.state("box_overflow")[0] == 0
    if channels == 3:
        assert got.shape == (T, rows, cols, 3)
        assert np.array_equal(got[..., 0], got[..., 1]) and np.array_equal(got[..., 0], got[..., 2])
        got = got[..., 0]
    assert np.array_equal(got, f["images"]), np.nonzero((got != f["images"]).any((1, 2)))[0][:8]


def test_cpp_class_through_frame_processor(tmp_path):
    """bgs_demo with FrameProcessor's enableMultiCueBGS on the fixture's clip of the constructor's defaults, 25 frames of 240 x 320: the
    first channel of every 8UC3 mask is the reference's image, zero for the 21 training frames and not afterwards, and the class has
    written its one-key XML."""
    from test_gpu_01_host_cpp import DEMO, HOST, write_fp_config
    f = FIX["step"]["step_defaults"]
    frames = f["frames"]
    n, rows, cols = frames.shape[:3]
    assert (n, rows, cols, f["train"]) == (25, 240, 320, 21) and f["params"] == dict(mc.DEFAULTS)
    subprocess.run(["make", "-s", "-C", HOST], check=True)
    wd = tmp_path
    frames.tofile(str(wd / "frames.raw"))
    write_fp_config(str(wd / "config"), set())
    path = wd / "config" / "FrameProcessor.xml"
    path.write_text(path.read_text().replace("</opencv_storage>", "<enableMultiCueBGS>1</enableMultiCueBGS>\n</opencv_storage>"))
    res = subprocess.run([DEMO, str(wd / "frames.raw"), str(rows), str(cols), str(n), str(wd / "out")], cwd=str(wd), capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    got = np.fromfile(str(wd / "out.MultiCueBGS.raw"), np.uint8).reshape(n, rows, cols)
    assert [mc.crc(im) for im in got] == list(f["image_crc"])
    assert not got[:21].any() and all(im.any() for im in got[21:])
    assert (wd / "config" / "MultiCueBGS.xml").read_text() == '<?xml version="1.0"?>\n<opencv_storage>\n<showOutput>1</showOutput>\n</opencv_storage>\n'
