"""The box stage and the whole-frame step of SJN_MultiCueBGS (bgs_multicue_boxes_device, bgs_multicue_process_device) on
the GPU against what the reference's own, unmodified SJN_MultiCueBGS.cpp computed (tests/golden/multicue_box_ref.npz, read through
tests/multicue_box_numpy.py; nothing here needs the reference tree) and against the numpy restatement beyond the fixture.  Every
comparison is byte for byte or bit for bit, and the sticky "overflow" and "box_overflow" counters are 0 in every parity run."""
import functools

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


def device_boxes(rh, rw, landmarks, frames):
    """landmarks [S][rh][rw], frames [S][rows][cols][3] -> numpy (fore, ghost, update, count, boxes, box_overflow)"""
    torch = _torch()
    with MultiCueModel(params_of(geometry(rh, rw)), n_streams=len(landmarks)) as m:
        out = m.boxes(torch.from_numpy(np.ascontiguousarray(landmarks)).cuda(), torch.from_numpy(np.ascontiguousarray(frames)).cuda())
        out = [t.cpu().numpy() for t in out]
        over = int(m.state("box_overflow")[0])
        assert m.state("count")[0] == 0  # the box stage does not touch the model
    return (*out, over)


def same_as(got, s, want_maps, want_boxes, where):
    fore, ghost, update, count, boxes, over = got
    assert over == 0, where
    assert count[s] == len(want_boxes) <= mb.MAX_BOXES, (where, "count", int(count[s]), len(want_boxes))
    assert np.array_equal(boxes[s], mb.box_rows(want_boxes)), (where, "boxes", np.nonzero((boxes[s] != mb.box_rows(want_boxes)).any(1))[0][:8])
    assert set(np.unique(fore[s])) <= {0, 255} and np.array_equal(fore[s] != 0, want_maps[0] != 0), (where, "fore")
    assert np.array_equal(ghost[s], want_maps[1]), (where, "ghost")
    assert np.array_equal(update[s], want_maps[2]), (where, "update")


@pytest.mark.parametrize("case", list(FIX["post"]))
def test_boxes_match_reference_fixture(case):
    """The reference's PostProcessing on the hand-made maps: blobs at 16 x 12, 40 x 30, 70 x 17 and 160 x 120 (a 39 x 52 frame, where the
    two nearest-neighbour rules read different pixels, and a 96 x 80 one), the largest window (the LDS limit), exactly 300 boxes."""
    f = FIX["post"][case]
    rh, rw = f["landmark"].shape
    got = device_boxes(rh, rw, f["landmark"][None], f["frame"][None])
    same_as(got, 0, (f["fore"], f["ghost"], f["update"]), f["boxes"], case)


SEEDED = [(12, 16, 24, 32, 131), (30, 40, 45, 70, 132), (17, 70, 40, 150, 133), (120, 160, 39, 52, 134), (120, 160, 80, 96, 135)]


@functools.lru_cache(maxsize=None)
def seeded(rh, rw, rows, cols, seed):
    lm = mb.blob_landmark(rh, rw, seed, blobs=8)
    frame = mb.blob_frame(rows, cols, lm, seed)
    r = mb.boxes(lm, frame)
    assert r["count"] <= mb.MAX_BOXES
    return lm, frame, r


@pytest.mark.parametrize("rh,rw,rows,cols,seed", SEEDED)
def test_boxes_match_restatement_on_seeded_blobs(rh, rw, rows, cols, seed):
    lm, frame, r = seeded(rh, rw, rows, cols, seed)
    got = device_boxes(rh, rw, lm[None], frame[None])
    same_as(got, 0, (r["fore"], r["ghost"], r["update"]), r["boxes"], seed)


def test_three_streams_in_one_object():
    runs = [seeded(30, 40, 45, 70, s) for s in (141, 142, 132)]
    got = device_boxes(30, 40, np.stack([r[0] for r in runs]), np.stack([r[1] for r in runs]))
    for s, (lm, frame, r) in enumerate(runs):
        same_as(got, s, (r["fore"], r["ghost"], r["update"]), r["boxes"], s)
        one = device_boxes(30, 40, lm[None], frame[None])
        for a, b in zip(got[:5], one[:5]):
            assert np.array_equal(a[s], b[0]), s


def test_301_blocks_drop_the_last_and_raise_the_counter():
    lm = mb.grid_landmark(120, 160, mb.MAX_BOXES + 1)
    frame = mb.blob_frame(120, 160, lm, 151)
    r = mb.boxes(lm, frame)
    assert r["count"] == mb.MAX_BOXES + 1 and len(r["boxes"]) == mb.MAX_BOXES
    fore, ghost, update, count, boxes, over = device_boxes(120, 160, lm[None], frame[None])
    assert np.array_equal(boxes[0], r["boxes"]) and over == 1


def device_process(p, scenes):
    """scenes: one [T][rows][cols][3] array per stream.  Returns (images [T][S][rows][cols], one dict of state planes per stream)."""
    torch = _torch()
    S, T = len(scenes), len(scenes[0])
    images = []
    with MultiCueModel(params_of(p), n_streams=S) as m:
        for t in range(T):
            images.append(m.process(torch.from_numpy(np.stack([s[t] for s in scenes])).cuda()).cpu().numpy())
        states = [{k: m.state(k, s) for k in mc.PLANES + ("box_overflow",)} for s in range(S)]
    return np.array(images), states


@pytest.mark.parametrize("case", list(FIX["step"]))
def test_process_matches_reference_fixture(case):
    f = FIX["step"][case]
    images, states = device_process(f["params"], [f["frames"]])
    st = states[0]
    assert not images[:f["train"]].any()  # training frames give zeros
    bad = [t for t in range(len(images)) if mc.crc(images[t, 0]) != f["image_crc"][t]]
    assert not bad, ("output images differ at frames", bad[:8])
    if f["images"] is not None:
        assert np.array_equal(images[:, 0], f["images"])
    for k in mc.STATE_PLANES:
        assert mc.crc(st[k]) == f["plane_crc"][k], k
    assert st["overflow"][0] == 0 and st["box_overflow"][0] == 0 and st["count"][0] == f["params"]["training_period"] + 2


def test_process_matches_restatement_on_a_seeded_scene():
    p = geometry(30, 40, **mc.FAST)
    train = p["training_period"] + 1
    frames = sc.frames_of("scripted", 60, 85, 30, train, 161)
    step = mb.Step(p)
    want = np.array([step.process(f) for f in frames])
    assert step.box_overflow == 0 and want[train:].any()
    images, states = device_process(p, [frames, frames[::-1].copy()])  # a second stream, so that the first is not alone in the launches
    assert np.array_equal(images[:, 0], want), np.nonzero((images[:, 0] != want).any((1, 2)))[0][:8]
    assert not images[:train].any()
    st, ws = states[0], step.m.state()
    for k in mc.PLANES:
        assert st[k].tobytes() == np.ascontiguousarray(ws[k]).tobytes(), k
    assert st["overflow"][0] == 0 and st["box_overflow"][0] == 0


def test_error_codes():
    torch = _torch()
    p = geometry(12, 16, **mc.FAST)
    f = torch.zeros((1, 37, 53, 3), dtype=torch.uint8, device="cuda")
    lm = torch.zeros((1, 12, 16), dtype=torch.uint8, device="cuda")

    def code(call, *a, **kw):
        with pytest.raises(capi.BgsError) as e:
            call(*a, **kw)
        return e.value.code

    with MultiCueModel(params_of(p)) as m:
        m.boxes(lm, f)  # fixes the geometry as a training call would
        assert code(m.boxes, lm, torch.zeros((1, 36, 53, 3), dtype=torch.uint8, device="cuda")) == capi.ERR_GEOMETRY
        assert code(m.process, torch.zeros((1, 37, 54, 3), dtype=torch.uint8, device="cuda")) == capi.ERR_GEOMETRY
        for _ in range(p["training_period"] + 1):
            assert not m.process(f).any()
        assert m.state("count")[0] == p["training_period"] + 2
        assert code(m.process, torch.zeros((1, 37, 54, 3), dtype=torch.uint8, device="cuda")) == capi.ERR_GEOMETRY
        m.landmark(f)
        assert code(m.process, f) == capi.ERR_STATE  # a bare landmark call without its updates
        um = torch.ones((1, 12, 16), dtype=torch.uint8, device="cuda")
        m.update(um, ghost=True)
        m.update(um)
        out = m.process(f)
        assert out.shape == (1, 37, 53) and not out.any()  # a constant scene has no foreground
        assert m.state("overflow")[0] == 0 and m.state("box_overflow")[0] == 0
