"""IndependentMultimodalBGS's area filter on the GPU (imbs_area_* / imbs_final_kernel of kernel_imbs.h over kernel_cc.h's two
labellings) against its definition, the contour follower of tests/imbs_numpy.py, on masks chosen to be hard: the
clips of tests/imbs_masks.py learn a constant background and then paint one mask a frame, so the plane that reaches the filter is
the painted mask (tests/test_imbs_cpu.py asserts that, and what the masks are made of, from the restatement alone).

Everything is compared byte for byte with imbs_numpy.run(..., area_filter=area_filter_follower): masks, backgrounds, the control
scalars after every frame, the packed words (made from the byte masks) and the state planes at the end.  A failing frame names its
generator, the size, the number of differing pixels and the first of them."""
import numpy as np
import pytest

import imbs_masks as mk
import imbs_numpy as im
from gpu_helpers import _torch
from test_gpu_21_imbs import BOTH, engine, same_state, state_of, words_of

pytestmark = pytest.mark.gpu

NCTL = len(im.CONTROL)
EDGE_33x70 = mk.edge_min_area(im.area_filter_follower_many(dict(mk.masks_for(33, 70))["noise45"], [])[1], 33 * 70)  # an area that occurs there
HOST_CASES = [(s, 2.5) for s in mk.SIZES + ((3, 3), mk.RECT_SIZE)] + [((33, 70), a) for a in (0.0, 30.0, EDGE_33x70)]


def frame_name(ref, t):
    return ref["names"][t - ref["first"]] if t >= ref["first"] else "the constant lead-in"


def check_frame(got, want, ref, t, where):
    bad = np.argwhere(np.asarray(got) != want)
    if len(bad):
        H, W = want.shape
        pytest.fail("%s: generator %s, %d x %d, minArea %g, frame %d: %d pixels differ, the first at (y, x) = (%d, %d): engine %d, follower %d"
                    % (where, frame_name(ref, t), H, W, ref["params"]["minArea"], t, len(bad), bad[0][0], bad[0][1], got[tuple(bad[0])], want[tuple(bad[0])]))


def want_state(ref):
    mdl = ref["out"][3]
    return dict(mdl.planes(), control=mdl.control())


def host_and_batch(ref):
    """The clip through the host path of one engine and, frame by frame, through the device batch path of another: masks,
    backgrounds, control scalars after every frame, packed words, the state at the end."""
    torch = _torch()
    frames, p = ref["frames"], ref["params"]
    want_masks, want_bgs, want_ctl, _ = ref["out"]
    T, H, W = frames.shape[:3]
    n, Wd = H * W, (H * W + 63) // 64
    host, dev = engine(p), engine(p)
    dev.set_geometry(H, W, 3)
    for t, f in enumerate(frames):
        fg, bg = host.process(f, want_bg=True)
        assert fg is not None and bg is not None and host.stream_flags(0) == BOTH
        check_frame(fg, want_masks[t], ref, t, "host path")
        assert np.array_equal(bg, want_bgs[t]), ("host path: background", frame_name(ref, t), t)
        ctl = host.get_state("control", (NCTL,), np.float64)
        assert ctl.tobytes() == want_ctl[t].tobytes(), ("control scalars", frame_name(ref, t), t, dict(zip(im.CONTROL, ctl)), dict(zip(im.CONTROL, want_ctl[t])))
        d = torch.from_numpy(np.array(f)).cuda().unsqueeze(0)  # the shared reference is read-only
        d_fg = torch.full((1, H, W), 9, dtype=torch.uint8, device="cuda")
        d_bg = torch.full((1, H, W, 3), 9, dtype=torch.uint8, device="cuda")
        d_bits = torch.full((1, Wd), -1, dtype=torch.int64, device="cuda")
        assert dev.process_batch_device(d, d_fg, d_bg, d_bits) == BOTH
        torch.cuda.synchronize()
        check_frame(d_fg.cpu().numpy()[0], want_masks[t], ref, t, "batch path")
        assert np.array_equal(d_bg.cpu().numpy()[0], want_bgs[t]), ("batch path: background", frame_name(ref, t), t)
        assert np.array_equal(d_bits.cpu().numpy().view(np.uint64)[0], words_of(want_masks[t], Wd)), ("packed words", frame_name(ref, t), t)
    same_state(state_of(host, p, n), want_state(ref), "host path against the restatement")
    same_state(state_of(dev, p, n), want_state(ref), "batch path against the restatement")
    host.close(), dev.close()


@pytest.mark.parametrize("size,min_area", HOST_CASES, ids=["%dx%d-a%g" % (s + (a,)) for s, a in HOST_CASES])
def test_every_generator_through_the_host_and_the_batch_path(size, min_area):
    ref = mk.reference(size[0], size[1], min_area)
    assert len(ref["names"]) == len(mk.NAMES) + 2 * (size == mk.RECT_SIZE)
    host_and_batch(ref)


@pytest.mark.parametrize("size", [(33, 70), (65, 131)], ids=lambda s: "%dx%d" % s)
def test_morphological_filtering_in_front_of_the_filter(size):
    """morphologicalFiltering = 1 on the noise and checkerboard masks, and on the corner blobs and the blobs on the image frame, of
    which the opening leaves something: the four morph_box_kernel launches over several tiles, cells outside the image taking no
    part, with the area filter behind them."""
    names = ("noise30", "noise45", "checkerboard", "corners", "frame_blobs")
    ref = mk.reference(size[0], size[1], 2.5, morph=1, only=names)
    painted, opened = [int(m.sum()) for m in ref["masks"]], [int(pl.sum()) for pl in ref["planes"]]
    left = [int((m == 255).sum()) for m in ref["out"][0][ref["first"]:]]
    assert opened[2] == 0 and all(0 < o < q for o, q in zip(opened[3:], painted[3:])) and 0 < left[3] < opened[3] and 0 < left[4] < opened[4], (painted, opened, left)
    host_and_batch(ref)


STREAMS = (("empty", "comb"), ("serpentine", "rings2"), ("noise30", "checkerboard"))  # what the three streams carry in the two injected frames


def test_streams_with_different_masks_in_one_call_do_not_mix():
    """Three streams of 33 x 70 whose frames carry different masks: first the empty mask beside the serpentine, then the pitch-2
    rings beside the checkerboard.  Every stream equals the restatement of its own clip (and so its own single-stream run): no label,
    share or parent crosses a stream boundary in the stacked labelling.  Once as one batch call a frame, once as two ranges (stream 0;
    streams 1 and 2) on two HIP streams."""
    torch = _torch()
    H, W, S = 33, 70, 3
    n, Wd = H * W, (H * W + 63) // 64
    refs = [mk.reference(H, W, 2.5, only=names) for names in STREAMS]
    p = refs[0]["params"]
    T = len(refs[0]["frames"])
    assert refs[0]["names"][0] == "empty" and refs[1]["names"] == ["serpentine", "rings2"] and refs[2]["names"][1] == "checkerboard"
    assert refs[0]["out"][0][-1].any() and not refs[0]["out"][0][-2].any() and refs[1]["out"][0][-2].any() and refs[1]["out"][0][-1].any()
    batch, ranges = engine(p, n_streams=S), engine(p, n_streams=S)
    batch.set_geometry(H, W, 3), ranges.set_geometry(H, W, 3)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for t in range(T):
        d = torch.from_numpy(np.stack([r["frames"][t] for r in refs])).cuda()
        outs = []
        for how in ("one batch call", "two ranges on two HIP streams"):
            d_fg = torch.full((S, H, W), 9, dtype=torch.uint8, device="cuda")
            d_bg = torch.full((S, H, W, 3), 9, dtype=torch.uint8, device="cuda")
            d_bits = torch.full((S, Wd), -1, dtype=torch.int64, device="cuda")
            if how == "one batch call":
                assert batch.process_batch_device(d, d_fg, d_bg, d_bits, first=0, count=S) == BOTH
            else:
                torch.cuda.current_stream().synchronize()
                ranges.process_batch_device(d[:1], d_fg[:1], d_bg[:1], d_bits[:1], hip_stream=s1.cuda_stream, first=0, count=1)
                ranges.process_batch_device(d[1:], d_fg[1:], d_bg[1:], d_bits[1:], hip_stream=s2.cuda_stream, first=1, count=2)
                s1.synchronize(), s2.synchronize()
            torch.cuda.synchronize()
            outs.append((how, d_fg.cpu().numpy(), d_bg.cpu().numpy(), d_bits.cpu().numpy().view(np.uint64)))
        for how, fg, bg, bits in outs:
            for s, r in enumerate(refs):
                check_frame(fg[s], r["out"][0][t], r, t, "%s, stream %d" % (how, s))
                assert np.array_equal(bg[s], r["out"][1][t]), (how, s, t)
                assert np.array_equal(bits[s], words_of(r["out"][0][t], Wd)), (how, s, t)
    for s, r in enumerate(refs):
        same_state(state_of(batch, p, n, stream=s), want_state(r), "one batch call, stream %d" % s)
        same_state(state_of(ranges, p, n, stream=s), want_state(r), "two ranges, stream %d" % s)
    batch.close(), ranges.close()


def test_one_clip_call_over_all_injected_frames():
    """33 x 70: the lead-in as one clip call, every injected frame in a second one."""
    torch = _torch()
    H, W = 33, 70
    ref = mk.reference(H, W, 2.5)
    frames, p, first = ref["frames"], ref["params"], ref["first"]
    want_masks, want_bgs = ref["out"][0], ref["out"][1]
    n, Wd = H * W, (H * W + 63) // 64
    d_all = torch.from_numpy(np.array(frames)).cuda().unsqueeze(1)  # [T][1][H][W][3]
    eng = engine(p)
    eng.set_geometry(H, W, 3)
    for lo, hi in ((0, first), (first, len(frames))):
        k = hi - lo
        d_fg = torch.full((k, 1, H, W), 9, dtype=torch.uint8, device="cuda")
        d_bg = torch.full((k, 1, H, W, 3), 9, dtype=torch.uint8, device="cuda")
        d_bits = torch.full((k, 1, Wd), -1, dtype=torch.int64, device="cuda")
        assert eng.process_clip_device(d_all[lo:hi], k, d_fg, d_bg, d_bits) == [BOTH] * k
        torch.cuda.synchronize()
        fg, bits = d_fg.cpu().numpy()[:, 0], d_bits.cpu().numpy().view(np.uint64)[:, 0]
        for i in range(k):
            check_frame(fg[i], want_masks[lo + i], ref, lo + i, "clip call")
            assert np.array_equal(bits[i], words_of(want_masks[lo + i], Wd)), lo + i
        assert np.array_equal(d_bg.cpu().numpy()[:, 0], want_bgs[lo:hi])
    same_state(state_of(eng, p, n), want_state(ref), "clip calls against the restatement")
    eng.close()
